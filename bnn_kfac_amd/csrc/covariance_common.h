// What covariance.hip (kfac_kron_cov) and covariance_outer.hip (kfac_kron_cov_outer)
// share: the limits of one call, the operand views, and the bodies of the two kernels
// both routes run -- a 64x64 tile of (tall matrix) x K2, and one K segment of a sample's
// nc x nc Gram block.
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

}  // namespace kfac
