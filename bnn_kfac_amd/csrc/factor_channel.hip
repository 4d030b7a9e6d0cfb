// The two kernels for the G factor of a conv layer (CHANNEL operand) with n <= 32.
#include "bf16x3.h"
#include "factor_common.h"

namespace kfac {

// Channel-major factors with n <= 8 (the G of a conv layer with few output
// channels, e.g. LeNet-5's conv1: 6): F = sum over (image, position) of g g^T is
// n(n+1)/2 FMAs per position against n loads -- an HBM stream, not MFMA work.  Each
// thread takes runs of 4 positions of the task's images (float4 loads, coalesced
// along positions, no LDS staging), keeps the lower triangle in registers, and the
// workgroup sums it in a fixed order (wave shuffles, then the 4 waves) into the
// same 16x16 slab / accumulator block the MFMA kernel writes.  (n = 9..16 stays on
// the MFMA kernel: 136 partial sums per thread cost more to reduce than they save.)
template <int NMAX>
__global__ __launch_bounds__(NTHREADS) void kfac_factor_channel_small(FactorArgs args, ConvGeom cg) {
  constexpr int NT = NMAX * (NMAX + 1) / 2;
  __shared__ float part[NTHREADS / 64][NT];
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int jx = 0;
  while (jx + 1 < args.njobs && task >= args.task_end[jx]) ++jx;
  const FactorJobDev& J = args.job[jx];
  const OpDev& op = J.x;
  const int split = task - J.task_begin;  // one unit: task = split
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = op.cols;
  const int64_t b0 = (int64_t)split * cg.B / J.splits, b1 = (int64_t)(split + 1) * cg.B / J.splits;
  // (image, 4-position run) pairs of the task: 32-bit index math (a task's pairs and a
  // job's images fit 32 bits; the 64-bit divisions cost as much issue as the FMAs)
  const uint32_t L4 = (uint32_t)(op.L >> 2), per = (uint32_t)(b1 - b0) * L4;
  float acc[NT];
#pragma unroll
  for (int e = 0; e < NT; ++e) acc[e] = 0.f;
  // PP (image, run) pairs per trip, their PP x n float4 loads issued together
  constexpr int PP = 2;
  auto src_of = [&](uint32_t q) {
    const uint32_t img = q / L4, r4 = q - img * L4;
    // image b0 + img of the job: batch seg of the queued batches, image bi in it
    const uint32_t ab = (uint32_t)b0 + img, seg = ab / (uint32_t)cg.bseg;
    return seg_base(J, args.segs, (int)seg) + (int64_t)(ab - seg * cg.bseg) * op.sB + 4 * r4;
  };
  for (uint32_t q = tid; q < per; q += PP * NTHREADS) {
    const float* sp[PP];
    bool ok[PP];
#pragma unroll
    for (int h = 0; h < PP; ++h) {
      ok[h] = h == 0 || q + h * NTHREADS < per;
      sp[h] = ok[h] ? src_of(q + h * NTHREADS) : sp[0];
    }
    floatx4 x[PP][NMAX];
#pragma unroll
    for (int c = 0; c < NMAX; ++c)
#pragma unroll
      for (int h = 0; h < PP; ++h) {
        const bool in = c < n;  // (channels past n: zero rows of the triangle)
        x[h][c] = in ? *reinterpret_cast<const floatx4*>(sp[h] + c * op.L) : floatx4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
    for (int h = 1; h < PP; ++h)
      if (!ok[h]) {
#pragma unroll
        for (int c = 0; c < NMAX; ++c) x[h][c] = floatx4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
    for (int h = 0; h < PP; ++h)
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0, e = 0; i < NMAX; ++i)
#pragma unroll
          for (int j = 0; j <= i; ++j, ++e) acc[e] = fmaf(x[h][i][u], x[h][j][u], acc[e]);
  }
#pragma unroll
  for (int e = 0; e < NT; ++e) {
    float v = acc[e];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) part[wave][e] = v;
  }
  __syncthreads();
  float* out = J.slab + (size_t)split * TILE * TILE;  // block 0 of tile 0
  for (int e = tid; e < NT; e += NTHREADS) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= e) ++i;
    const int j = e - i * (i + 1) / 2;
    const float t = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
    float* at1 = &out[i * TILE + j];
    float* at2 = &out[j * TILE + i];
    if (!J.accum) {
      *at1 = t;
      *at2 = t;
    } else {
      const float v = J.sbeta == 0.f ? J.alpha * t : fmaf(J.sbeta, *at1, J.alpha * t);
      *at1 = v;
      *at2 = v;
    }
  }
}

// Channel-major factors with 8 < n <= 32 (LeNet-5's conv2 G: 16 channels x 100
// positions per image) in bf16x3, fragments straight from HBM: a channel's positions
// are contiguous, so a lane's fragment -- 8 consecutive positions of one channel -- is
// two float4 loads, split in registers (x3_split8); one 32 x 32 diagonal block, four
// MFMAs per 16 positions (x3_four).  Each wave takes whole images (images w, w + 4, ..
// of the task), its k-steps flattened over them with XC_D k-steps of loads in flight;
// the 4 waves' sums meet in LDS in wave order, then acc + acc2 + acc2^T.  (It replaces
// the LDS-staged fp32 kernel there: an HBM stream at 2.2 TB/s.)
constexpr int XC_D = 4;  // k-steps of loads in flight per wave
__global__ __launch_bounds__(NTHREADS) void kfac_factor_channel_x3(FactorArgs args, ConvGeom cg) {
  __shared__ float red[2 * (NTHREADS / 64 - 1)][16][64];
  __shared__ float tr[32][33];
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int jx = 0;
  while (jx + 1 < args.njobs && task >= args.task_end[jx]) ++jx;
  const FactorJobDev& J = args.job[jx];
  const OpDev& op = J.x;
  const int split = task - J.task_begin;  // one unit: task = split
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = op.cols, L = (int)op.L, m = lane & 31, hh = lane >> 5;
  const int64_t b0 = (int64_t)split * cg.B / J.splits, b1 = (int64_t)(split + 1) * cg.B / J.splits;
  const int nks = (L + 15) / 16;
  const int nimg = b1 - b0 > wave ? (int)((b1 - b0 - wave + 3) / 4) : 0;
  const int total = nimg * nks;  // this wave's k-steps
  // cursor of the next k-step to load: image j of the wave, k-step t; its channel row
  const float* rowp = nullptr;
  int j = 0, t = 0;
  auto image_row = [&](int jj) __attribute__((always_inline)) {
    const uint32_t ab = (uint32_t)(b0 + wave + 4 * (int64_t)jj), seg = ab / (uint32_t)cg.bseg;
    return seg_base(J, args.segs, (int)seg) + (int64_t)(ab - seg * cg.bseg) * op.sB + (int64_t)min(m, n - 1) * L;
  };
  if (total > 0) rowp = image_row(0);
  auto load = [&](float (&x)[8]) __attribute__((always_inline)) {
    const int p = 16 * t + 8 * hh;
    const bool r0 = m < n && p < L, r1 = m < n && p + 4 < L;
    const floatx4 lo = r0 ? *reinterpret_cast<const floatx4*>(rowp + p) : floatx4{0.f, 0.f, 0.f, 0.f};
    const floatx4 hi = r1 ? *reinterpret_cast<const floatx4*>(rowp + p + 4) : floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      x[e] = lo[e];
      x[4 + e] = hi[e];
    }
    if (++t == nks) {
      t = 0;
      if (++j < nimg) rowp = image_row(j);
      else j = nimg;
    }
  };
  floatx16 acc, acc2;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = acc2[v] = 0.f;
  // ring of XC_D k-steps: step s multiplies slot s % XC_D, then reloads it for s + XC_D
  // (unconditionally: past the wave's last k-step the cursor re-reads its last image,
  // unused -- a conditional load made every wait vmcnt(0))
  if (total > 0) {
    float x[XC_D][8];
#pragma unroll
    for (int d = 0; d < XC_D; ++d) load(x[d]);
    int s = 0;
    for (; s + XC_D <= total; s += XC_D) {
#pragma unroll
      for (int d = 0; d < XC_D; ++d) {
        const X3Frag f = x3_split8(x[d]);
        load(x[d]);
        x3_four(acc, acc2, f);
      }
    }
#pragma unroll
    for (int d = 0; d < XC_D; ++d)
      if (s + d < total) x3_four(acc, acc2, x3_split8(x[d]));
  }
  // the 4 waves' sums in wave order (deterministic), then acc + acc2 + acc2^T
  if (wave > 0)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      red[2 * (wave - 1)][v][lane] = acc[v];
      red[2 * (wave - 1) + 1][v][lane] = acc2[v];
    }
  __syncthreads();
  if (wave > 0) return;
  for (int w = 0; w < NTHREADS / 64 - 1; ++w)
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      acc[v] += red[2 * w][v][lane];
      acc2[v] += red[2 * w + 1][v][lane];
    }
#pragma unroll
  for (int v = 0; v < 16; ++v) tr[acc_row(v, lane)][m] = acc2[v];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] += acc2[v] + tr[m][acc_row(v, lane)];
  float* out = J.slab + (size_t)split * TILE * TILE;  // block (0, 0) of slab tile 0
  put_partial(J, acc, [&](int v) { return &out[acc_row(v, lane) * TILE + m]; });
}

// ------------------------------------------------------------------- host side
// the register-triangle kernel takes channel factors with n <= 8 (an n = 16 instance --
// 136 sums per thread, 256 VGPRs -- ran LeNet-5's conv2 G at 0.63 ms per pass against
// 0.17 on the MFMA kernel, `profiles/r06z10/`).  KFAC_CONV_SMALL=0: those factors on the
// MFMA kernel (A/B checks)
bool channel_small(const ConvGeom& g) { return knobs().conv_small && g.n <= 8; }

// kfac_factor_channel_x3 takes a CHANNEL operand conv_fp32_geom accepted (float4-shaped,
// aligned images) with 8 < n <= 32: one task per K-split
bool channel_x3_geom(const kfac_operand& o, ConvGeom& g) {
  if (o.layout != KFAC_CHANNEL || g.n <= 8 || g.n > 32 || !knobs().conv_x3) return false;
  g.units = 1;
  return true;
}

int launch_channel_x3(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream) {
  hipLaunchKernelGGL(kfac_factor_channel_x3, dim3(tasks), dim3(NTHREADS), 0, stream, args, g);
  return KFAC_OK;
}

int launch_channel_small(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream) {
  // the exact channel count (LeNet-5 conv1: 6) sizes the register triangle and its
  // reduction; other counts take the next instance up (their extra rows are zero)
  if (g.n == 6)
    hipLaunchKernelGGL(kfac_factor_channel_small<6>, dim3(tasks), dim3(NTHREADS), 0, stream, args, g);
  else if (g.n <= 4)
    hipLaunchKernelGGL(kfac_factor_channel_small<4>, dim3(tasks), dim3(NTHREADS), 0, stream, args, g);
  else
    hipLaunchKernelGGL(kfac_factor_channel_small<8>, dim3(tasks), dim3(NTHREADS), 0, stream, args, g);
  return KFAC_OK;
}

}  // namespace kfac
