// What covariance.hip (kfac_kron_cov) and covariance_outer.hip (kfac_kron_cov_outer)
// share: the limits of one call, the operand views, and the bodies of the two kernels
// both routes run -- a 64x64 tile of (tall matrix) x K2, and one K segment of a sample's
// nc x nc Gram block -- and what their damping sweeps share: the weight views and the
// weighted Gram of a staged segment for a group of grid points.
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
  const float* wG;  // nt x nG
  int64_t ldwA, ldwG;
};
struct SweepArgs {
  int ntau;
  SweepWeights job[CMAXJ];
};

// Weighted Gram partials of one sample over the K segment [k0, k0 + WSEG): for every grid
// point tau, part[tau * part_stride] (nc x nc, lower triangle written) =
//   sum_k w_tau[k] Tb[c][k] Tb[c'][k] ,
//   w_tau[k] = wA_tau[k / nG] * wG_tau[k % nG] (DENSE)  or  wG_tau[k] (K = nG).
// The sample's nc row segments are staged ONCE ([k][c], thread t owns k0 + t and its
// (a, g): one division per thread, none in a loop); the grid points then go through in
// groups of WTG on the staged data: a group's weights are staged beside the segment, and
// each tau owns an accumulator that takes the wave's quarter of the segment in k order
// (the B fragment scaled by its k-row's weight: one multiply per MFMA and tau), so slice
// tau does not depend on nt or on its place in the group.  The four wave partials are
// summed in cov_gram_segment's fixed order.  Loads are unconditional (clamped index).
template <bool DENSE>
__device__ __forceinline__ void cov_wgram_segment(const float* Tb, int64_t K, int nc, int64_t k0,
                                                  const SweepWeights& W, int nG, int nt, float* part,
                                                  int64_t part_stride, float* lds) {
  float* xs = lds;
  float* wl = xs + WSEG * WPITCH;
  float* red = wl + WTG * WSEG;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = lane >> 5, rr = lane & 31;
  const bool live = k0 + tid < K;
  const int64_t kc = live ? k0 + tid : K - 1;
  const float* src = Tb + kc;
#pragma unroll 8
  for (int c = 0; c < 32; ++c) {
    const float x = src[(int64_t)min(c, nc - 1) * K];
    xs[tid * WPITCH + c] = (live && c < nc) ? x : 0.f;
  }
  int64_t ia = 0, ig = kc;
  if (DENSE) {
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
      if (DENSE) w *= W.wA[tt * W.ldwA + ia];
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

}  // namespace kfac
