// Conv2d Jacobian rows for the GLM predictive, formed on the device.
//
// A Conv2d layer's Jacobian row is a sum over the output positions: with patch_b the
// implicit im2col of the layer's input a_b (C x H x W; L = Ho*Wo positions p = oh*Wo + ow,
// cols = C*kh*kw features k in F.unfold's order) and D_{b,c} = d f_c(x_b) / d z (nG x L) at
// the layer's output,
//   M_{b,c}[k][g]    = sum_p patch_b[p][k] * D_{b,c}[g][p]      (k < cols)
//   M_{b,c}[cols][g] = sum_p D_{b,c}[g][p]                      (bias row: the ones column)
// stored as kfac_cov_job::J wants it: row r = b*nc + c at M + r*ldM, element k*nG + g.
// Per sample that is ONE GEMM (nA x L)(L x nc*nG) over all columns j = c*nG + g at once:
// the classes share the column axis (LeNet-5's conv1 fills 60 of a tile's 64 columns
// instead of 6) and a sample's patches are gathered once, not nc times.
//
// kfac_cov_conv_rows: one workgroup per (job, sample, 64-row a-tile, 64-column tile), tasks
// flat over the jobs in plain block order, a sample's tiles next to each other (they share
// its image and its D).  The body is contract_tile over k = p in [0, L): operand A is
// Panel<KFAC_PATCH> on sample b's image, operand B the panel of this file.  No split-K, no
// atomics: an element is one k-ordered fma chain from zero over its sample's positions, so
// two calls give the same bits and a row depends on a_b, D_{b,c} and the shapes only -- not
// on nb, nor on nc, nor on the tile its column falls in.  contract_tile's narrow mode would
// choose the summation order by nc*nG <= 32 and break the second property: not used.
#include "covariance_common.h"

namespace kfac {

constexpr int KFAC_CONVDELTA = 18;  // panel layout of [D_{b,0}^T | D_{b,1}^T | ...] (internal to this file)

// element (p, j) = ptr[(j / nG) * ldD + (j % nG) * L + p]: column j = c*nG + g is row g of
// D_{b,c}, contiguous in p.  rows = L, cols = nc*nG; nG travels in OpDev::C.
__device__ __forceinline__ OpDev convdelta_op(const float* p, int64_t L, int cols, int nG, int64_t ldD) {
  OpDev d{};
  d.ptr = p; d.layout = KFAC_CONVDELTA; d.rows = L; d.cols = cols; d.ld = ldD; d.L = L; d.C = nG;
  d.ones = -1;
  return d;
}

// Panel<CHANNEL>'s thread map (32 lanes walk p, contiguous in a row of D).  A thread's 8
// column offsets are fixed at init: no division in the stage loop.  Loads are
// unconditional: p is clamped to the last position and a column past the end to the last
// column, and what was clamped is zeroed afterwards.
template <>
struct Panel<KFAC_CONVDELTA> {
  static constexpr int PITCH = LDP;
  const float* base;
  int64_t kend;
  int64_t off[8];
  int r, c0;
  unsigned live;  // bit m: column c0 + 8 m exists
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0, int tid,
                                       int64_t k_end, int64_t) {
    base = base_; kend = k_end;
    r = tid & 31; c0 = tid >> 5;
    const int nG = op.C;
    live = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int j = col0 + c0 + 8 * m;
      const int jc = min(j, op.cols - 1);
      const int c = jc / nG;
      off[m] = (int64_t)c * op.ld + (int64_t)(jc - c * nG) * op.L;
      live |= (unsigned)(j < op.cols) << m;
    }
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
    const int64_t kk = k + r;
    const bool ok = kk < kend;
    const float* p = base + (ok ? kk : kend - 1);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const float x = p[off[m]];
      v[m] = (ok && ((live >> m) & 1u)) ? x : 0.f;
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 8; ++m) lds[r * LDP + c0 + 8 * m] = v[m];
  }
};

struct ConvRowsJobDev {
  OpDev x;         // KFAC_PATCH, rows = nb*L
  const float* D;  // sample b's class c at D + (b*nc + c)*ldD: nG x L
  float* M;        // row r = b*nc + c at M + r*ldM: nA x nG
  int64_t ldD, ldM;
  int nA, nG, ncols;  // nA = cols + ones, ncols = nc*nG
  int ct, per;        // column tiles, tiles per sample
  int begin;          // first task of this job
};

struct ConvRowsArgs {
  int njobs, nc;
  int end[CMAXJ];
  ConvRowsJobDev job[CMAXJ];
};
static_assert(sizeof(ConvRowsArgs) <= 4096, "kernel argument block");

__global__ __launch_bounds__(NTHREADS) void kfac_cov_conv_rows(ConvRowsArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const ConvRowsJobDev& C = args.job[cov_find_job(args.end, args.njobs, task)];
  const int local = task - C.begin;
  const int64_t b = local / C.per;
  const int t = local - (int)b * C.per;
  const int a0 = (t / C.ct) * TILE, j0 = (t % C.ct) * TILE;
  OpDev x = C.x;
  x.ptr += b * x.sB;  // sample b alone: its positions are the K rows [0, L)
  const OpDev d = convdelta_op(C.D + b * args.nc * C.ldD, x.L, C.ncols, C.nG, C.ldD);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ai = a0 + (wave >> 1) * 32, jq = j0 + (wave & 1) * 32;
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // M[a][j] = sum_p patch[p][a] D[p][j]; a quadrant beyond nA or the last column sits out
  contract_tile<KFAC_PATCH, KFAC_CONVDELTA>(x, a0, d, j0, 0, x.L, false, ai < C.nA && jq < C.ncols,
                                            lds, acc);
  const int j = jq + (lane & 31);
  if (j >= C.ncols) return;
  const int c = j / C.nG, g = j - c * C.nG;
  float* dst = C.M + (b * args.nc + c) * C.ldM + g;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int a = ai + acc_row(v, lane);
    if (a < C.nA) dst[(int64_t)a * C.nG] = acc[v];
  }
}

static bool conv_rows_job_ok(const kfac_cov_conv_rows_job& q, int64_t nb) {
  const kfac_operand& x = q.x;
  const int64_t lim = (int64_t)1 << 31;
  if (!x.ptr || !q.D || !q.M || x.layout != KFAC_PATCH || q.nG <= 0) return false;
  if (x.C <= 0 || x.H <= 0 || x.W <= 0 || x.kh <= 0 || x.kw <= 0 || x.sh <= 0 || x.sw <= 0 ||
      x.ph < 0 || x.pw < 0 || x.Ho <= 0 || x.Wo <= 0)
    return false;
  if (x.kh >= 1 << 15 || x.kw >= 1 << 15) return false;  // the loader packs (ki << 16) | kj
  const int64_t chw = (int64_t)x.C * x.H * x.W;  // (H*W < 2^62, checked before the third factor)
  if ((int64_t)x.H * x.W >= lim || chw >= lim || x.sB < chw) return false;
  // every patch lies in the padded image (and oh*sh, ow*sw stay 32-bit)
  if ((int64_t)x.H + 2 * (int64_t)x.ph >= lim || (int64_t)x.W + 2 * (int64_t)x.pw >= lim) return false;
  if ((int64_t)(x.Ho - 1) * x.sh + x.kh > (int64_t)x.H + 2 * (int64_t)x.ph ||
      (int64_t)(x.Wo - 1) * x.sw + x.kw > (int64_t)x.W + 2 * (int64_t)x.pw)
    return false;
  if ((int64_t)x.cols != (int64_t)x.C * x.kh * x.kw) return false;
  if (x.L != (int64_t)x.Ho * x.Wo) return false;
  if (x.rows % x.L != 0 || x.rows / x.L != nb) return false;
  const int64_t nA = (int64_t)x.cols + (x.has_ones != 0);
  if (nA >= lim - TILE) return false;
  if (q.ldD / q.nG < x.L || q.ldM / q.nG < nA) return false;  // ldD >= nG*L, ldM >= nA*nG
  return true;
}

}  // namespace kfac

using namespace kfac;

extern "C" int kfac_cov_conv_rows(const kfac_cov_conv_rows_job* jobs, int njobs, int64_t nb, int nc,
                                  kfac_stream_t stream) {
  const int64_t lim = (int64_t)1 << 31;
  if (!jobs || njobs <= 0 || njobs > CMAXJ || nb <= 0 || nb >= lim || nc <= 0) return KFAC_EINVAL;
  ConvRowsArgs args{};
  args.njobs = njobs;
  args.nc = nc;
  int64_t ntasks = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_cov_conv_rows_job& q = jobs[i];
    if (!conv_rows_job_ok(q, nb)) return KFAC_EINVAL;
    const int64_t ncols = (int64_t)nc * q.nG;
    if (ncols >= lim - TILE) return KFAC_EINVAL;
    ConvRowsJobDev& d = args.job[i];
    d.x = to_dev(q.x);
    d.D = q.D; d.M = q.M; d.ldD = q.ldD; d.ldM = q.ldM;
    d.nA = q.x.cols + (q.x.has_ones != 0);
    d.nG = q.nG;
    d.ncols = (int)ncols;
    d.ct = (int)cdiv(ncols, TILE);
    const int64_t per = cdiv(d.nA, TILE) * d.ct;
    if (per >= lim) return KFAC_EINVAL;
    d.per = (int)per;
    d.begin = (int)ntasks;
    ntasks += nb * per;
    if (ntasks >= lim) return KFAC_EINVAL;
    args.end[i] = (int)ntasks;
  }
  hipLaunchKernelGGL(kfac_cov_conv_rows, dim3((unsigned)ntasks), dim3(NTHREADS), 0, (hipStream_t)stream,
                     args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}
