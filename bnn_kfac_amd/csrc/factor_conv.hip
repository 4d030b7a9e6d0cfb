#include <algorithm>

#include "factor_common.h"

namespace kfac {

// ------------------------------------------------------------ conv operands
// Conv2d factors with each image staged whole in LDS (replaces the per-element
// register gather of the im2col / channel-major panel loaders for images that fit).
// F = sum_rows P[row]^T P[row], row = (image b, output position):
//   PATCH   (A, implicit F.unfold): P[(oh,ow)][(c,ki,kj)] = x_pad[b][c][oh*sh+ki][ow*sw+kj]
//   CHANNEL (G, permute(1,0,2,3)):  P[pos][c] = g[b][c][pos]
// A task is a group of blocks over WHOLE images.  Each image is
// staged into LDS once (coalesced loads of the next image in flight meanwhile);
// zero padding, the bias ones column and tile padding live in planes filled once
// per task.  An MFMA's k-lanes take different output ROWS (PATCH: oh = g*KR + k;
// CHANNEL: contiguous position segments), so along a row every lane's operand is
// one LDS read at base_lane + t*stride: no per-MFMA index arithmetic (stride 1:
// immediate offsets).  Rows past Ho read the A operand from the zero plane.
//   n <= 16 : one 16x16 block, v_mfma_f32_16x16x4f32 (KR = 4), the 4 waves take
//             different row groups / segments;
//   n <= 32 : one 32x32 quadrant, 32x32x2 (KR = 2), split over waves the same way;
//   else    : the lower triangle in 32x32 blocks, 4*CONV_CB per workgroup (CONV_CB
//             per wave, balanced to one block; each image staged once for all).
// Partials go to the slab / accumulator tiles exactly as the other paths (block
// (bi, bj) = quadrant (bi & 1, bj & 1) of tile (bi / 2, bj / 2)).
constexpr int CONV_LDS_MAX = 12288;  // staged floats per workgroup (48 KB of LDS)

constexpr int CONV_CB = 2;  // 32x32 blocks per wave (CONV_BLOCKS): 4*CONV_CB per workgroup
// operand chunk of the two-block row loop: 2 steps ahead (4 MFMAs of 64 cycles cover the
// LDS latency) instead of 4 keeps the PATCH instances inside the 128-VGPR budget of 4
// workgroups per CU without spilling (LeNet-5: conv 2.90 vs 3.04 ms per pass, 1.69 vs
// 1.63e7 img/s, 3 alternating runs, profiles/r06b/)
constexpr int CONV_CK2 = 2;

template <int LAYOUT, int PMAXE, bool STRIDE1, int CB = CONV_CB, bool M3 = false>
__global__ __launch_bounds__(NTHREADS, (CB == 2 && !M3) ? KFAC_CONV_OCC : 4) void kfac_factor_conv(
    FactorArgs args, ConvGeom cg) {
  extern __shared__ __attribute__((aligned(16))) float cimg[];
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int jx = 0;
  while (jx + 1 < args.njobs && task >= args.task_end[jx]) ++jx;
  const FactorJobDev& J = args.job[jx];
  const OpDev& op = J.x;
  const int local = task - J.task_begin;
  const int unit = local / J.splits, split = local - unit * J.splits;  // unit: block group
  // wave index through readfirstlane: the block bookkeeping derived from it (same[],
  // nmine, the row groups) is then wave-uniform (scalar branches, no exec-mask
  // juggling around the operand reads of the MFMA chain)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // M3: the mode-3 instance (its three accumulators and operand rings stay out of the
  // other modes' register budget)
  const int mode = M3 ? 3 : cg.mode;
  const bool m16 = mode >= 2;  // 16x16x4 MFMA modes (2: one block; 3: blocks 00, 10, 11)
  const int klane = m16 ? lane >> 4 : lane >> 5;
  const int64_t b0 = (int64_t)split * cg.B / J.splits, b1 = (int64_t)(split + 1) * cg.B / J.splits;

  // staging map: source element (PATCH) / float4 (CHANNEL) q of this thread -> LDS index
  int dmap[PMAXE];
#pragma unroll
  for (int q = 0; q < PMAXE; ++q) {
    const int e = tid + q * NTHREADS;
    int d = -1;
    if (e < cg.src) {
      if (LAYOUT == KFAC_PATCH) {
        const int hw = op.H * op.W, c = e / hw, r = e - c * hw, h = r / op.W, w = r - h * op.W;
        d = c * cg.plane + (h + op.ph) * cg.Wp + (w + op.pw);
      } else {  // float index of the float4's first element (planes need not be 4-aligned)
        const int L4 = (int)op.L >> 2, c = e / L4;
        d = c * cg.plane + 4 * (e - c * L4);
      }
    }
    dmap[q] = d;
  }
  // next image in flight: PATCH stages single floats, CHANNEL float4s
  using PreT = std::conditional_t<LAYOUT == KFAC_PATCH, float, floatx4>;
  PreT pre[PMAXE];
  auto fetch = [&](int64_t b) {
    const int seg = (int)((uint32_t)b / (uint32_t)cg.bseg);
    const float* src = seg_base(J, args.segs, seg) + (b - (int64_t)seg * cg.bseg) * op.sB;
#pragma unroll
    for (int q = 0; q < PMAXE; ++q) {
      if (dmap[q] < 0) continue;
      if constexpr (LAYOUT == KFAC_PATCH) pre[q] = src[tid + q * NTHREADS];
      else pre[q] = reinterpret_cast<const floatx4*>(src)[tid + q * NTHREADS];
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int q = 0; q < PMAXE; ++q) {
      if (dmap[q] < 0) continue;
      if constexpr (LAYOUT == KFAC_PATCH) {
        cimg[dmap[q]] = pre[q];
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) cimg[dmap[q] + r] = pre[q][r];
      }
    }
  };

  // per-lane operand columns -> LDS offset of the column's plane position
  auto column = [&](int col) -> int {
    if (col >= op.cols) return (col == op.ones) ? cg.ones_base : cg.zero_base;
    if (LAYOUT == KFAC_PATCH) {
      const int kk = op.kh * op.kw, c = col / kk, r = col - c * kk, ki = r / op.kw;
      return c * cg.plane + ki * cg.Wp + (r - ki * op.kw);
    }
    return col * cg.plane;
  };
  // Blocks of this wave.  mode 0: the factor's lower triangle in 32x32 blocks
  // (b = tri index), 4*CB per workgroup (unit), block b = unit*4*CB + wave + 4i: the
  // workgroup stages each image once for all its blocks and the waves' shares differ
  // by at most one block.  Narrow modes: the one block, every wave.
  const int cl = m16 ? lane & 15 : lane & 31;
  int offA[CB], offB[CB], bij[CB];
  bool same[CB];
  int nmine = 0;
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    const int bidx = unit * 4 * CB + wave + 4 * i;
    int bi = 0, bj = 0;
    if (mode == 0) tri_decode(bidx, bi, bj);
    const bool mine = mode ? i == 0 : bidx < cg.nq;
    nmine += mine;
    // mode 3: offA[0] / offA[1] = feature columns 0..15 / 16..31 (both operands)
    offA[i] = column(mode == 3 ? 16 * i + cl : 32 * bi + cl);
    offB[i] = column(32 * bj + cl);
    same[i] = bi == bj;
    bij[i] = (bi << 16) | bj;
  }

  floatx16 acc[CB];
  floatx4 acc16, acc16b, acc16c;  // mode 2: block 00; mode 3: blocks 00, 10, 11
#pragma unroll
  for (int i = 0; i < CB; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;
#pragma unroll
  for (int v = 0; v < 4; ++v) acc16[v] = acc16b[v] = acc16c[v] = 0.f;

  // one row group of one block: T MFMAs, operands read two MFMAs ahead (LDS latency
  // off the accumulator chain)
  // Operands in chunks of CK steps, double-buffered: chunk c+1's LDS reads are issued
  // before chunk c's MFMAs, so each read has CK MFMAs (>= 128 cycles) to land.  (B is
  // read even where it equals A -- a diagonal block: one more LDS read, but no select
  // that would make the next MFMA wait for the read.)
  auto row_mfmas = [&](const float* pa, const float* pb, bool, auto mfma) {
    constexpr int CK = 4;
    const int st = STRIDE1 ? 1 : cg.stride, T = cg.T, last = (T - 1) * st;
    float ca[CK], cb[CK], na[CK], nb[CK];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      const int o = min(u * st, last);
      ca[u] = pa[o];
      cb[u] = pb[o];
    }
    for (int t0 = 0; t0 < T; t0 += CK) {
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        const int o = min((t0 + CK + u) * st, last);
        na[u] = pa[o];
        nb[u] = pb[o];
      }
#pragma unroll
      for (int u = 0; u < CK; ++u)
        if (t0 + u < T) mfma(ca[u], cb[u]);
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        ca[u] = na[u];
        cb[u] = nb[u];
      }
    }
  };
  // two blocks (CB = 2) of one row group: operands for CK steps of both blocks per
  // chunk, double-buffered as in row_mfmas, MFMAs alternating between the blocks
  auto row_mfmas2 = [&](const float* pa0, const float* pb0, const float* pa1, const float* pb1) {
    constexpr int CK = CONV_CK2;
    const int st = STRIDE1 ? 1 : cg.stride, T = cg.T, last = (T - 1) * st;
    float ca[2][CK], cb[2][CK], na[2][CK], nb[2][CK];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      const int o = min(u * st, last);
      ca[0][u] = pa0[o]; cb[0][u] = pb0[o];
      ca[1][u] = pa1[o]; cb[1][u] = pb1[o];
    }
    for (int t0 = 0; t0 < T; t0 += CK) {
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        const int o = min((t0 + CK + u) * st, last);
        na[0][u] = pa0[o]; nb[0][u] = pb0[o];
        na[1][u] = pa1[o]; nb[1][u] = pb1[o];
      }
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        if (t0 + u < T) {
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[0][u], cb[0][u], acc[0], 0, 0, 0);
          acc[CB - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[1][u], cb[1][u], acc[CB - 1], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        ca[0][u] = na[0][u]; cb[0][u] = nb[0][u];
        ca[1][u] = na[1][u]; cb[1][u] = nb[1][u];
      }
    }
  };
  // mode 3: features 0..15 (v0) and 16..31 (v1) of CK steps per chunk, double-
  // buffered; each step feeds three 16x16x4 MFMAs (blocks 00 = v0 v0, 10 = v1 v0,
  // 11 = v1 v1): two LDS reads per three MFMAs, where the 32x32 block of mode 1 took
  // two per MFMA and computed the strictly-upper quarter too
  auto row_mfmas3 = [&](const float* p0, const float* p1) {
    constexpr int CK = 4;
    const int st = STRIDE1 ? 1 : cg.stride, T = cg.T, last = (T - 1) * st;
    float c0[CK], c1[CK], n0[CK], n1[CK];
#pragma unroll
    for (int u = 0; u < CK; ++u) {
      const int o = min(u * st, last);
      c0[u] = p0[o];
      c1[u] = p1[o];
    }
    for (int t0 = 0; t0 < T; t0 += CK) {
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        const int o = min((t0 + CK + u) * st, last);
        n0[u] = p0[o];
        n1[u] = p1[o];
      }
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        if (t0 + u < T) {
          acc16 = __builtin_amdgcn_mfma_f32_16x16x4f32(c0[u], c0[u], acc16, 0, 0, 0);
          acc16b = __builtin_amdgcn_mfma_f32_16x16x4f32(c1[u], c0[u], acc16b, 0, 0, 0);
          acc16c = __builtin_amdgcn_mfma_f32_16x16x4f32(c1[u], c1[u], acc16c, 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < CK; ++u) {
        c0[u] = n0[u];
        c1[u] = n1[u];
      }
    }
  };
  // one row group of every block of this wave (rowA / rowB: LDS offsets added to the
  // blocks' column offsets; zeroA: A read from the zero plane)
  auto blocks = [&](int rowA, int rowB, bool zeroA) {
    if constexpr (M3) {  // both operands from the same reads: a row past Ho reads zeros
      row_mfmas3(cimg + (zeroA ? cg.zero_base : offA[0] + rowA),
                 cimg + (zeroA ? cg.zero_base : offA[CB - 1] + rowA));
      return;
    }
    if (mode == 2) {
      row_mfmas(cimg + (zeroA ? cg.zero_base : offA[0] + rowA), cimg + offB[0] + rowB, true,
                [&](float a, float b) { acc16 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc16, 0, 0, 0); });
      return;
    }
    if constexpr (CB == 2) if (nmine == 2) {
      // both blocks in one pass, their MFMAs alternating (two independent chains)
      row_mfmas2(cimg + (zeroA ? cg.zero_base : offA[0] + rowA), cimg + offB[0] + rowB,
                 cimg + (zeroA ? cg.zero_base : offA[1] + rowA), cimg + offB[1] + rowB);
      return;
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
      if (i >= nmine) break;
      row_mfmas(cimg + (zeroA ? cg.zero_base : offA[i] + rowA), cimg + offB[i] + rowB, same[i],
                [&](float a, float b) { acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[i], 0, 0, 0); });
    }
  };

  if (b0 < b1) fetch(b0);
  // constant planes (and the zero padding / segment tails of the image planes)
  for (int e = tid; e < cg.lds; e += NTHREADS)
    cimg[e] = (LAYOUT == KFAC_PATCH && e >= cg.ones_base && e < cg.zero_base) ? 1.f : 0.f;
  for (int64_t b = b0; b < b1; ++b) {
    __syncthreads();  // every wave done with the previous image (and the fill)
    commit();
    __syncthreads();
    if (b + 1 < b1) fetch(b + 1);  // next image's loads fly during the MFMAs
    if (nmine == 0) continue;
    if (LAYOUT == KFAC_PATCH) {
      for (int g = mode ? wave : 0; g < cg.G; g += mode ? 4 : 1) {
        const int oh = g * cg.KR + klane;  // rows past Ho: A from the zero plane
        blocks(oh * cg.rowstep, min(oh, cg.Ho - 1) * cg.rowstep, oh >= cg.Ho);
      }
    } else {
      const int sg = mode ? wave * cg.KR + klane : klane;
      blocks(sg * cg.rowstep, sg * cg.rowstep, false);
    }
  }

  float* out = J.slab + (size_t)split * TILE * TILE;  // narrow: tile 0
  if (mode == 1) {
    store_narrow(J, out, acc[0], cimg);
    return;
  }
  if constexpr (M3) {  // sum the 4 waves' three 16x16 partials in wave order (deterministic)
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        cimg[((wave - 1) * 12 + v) * 64 + lane] = acc16[v];
        cimg[((wave - 1) * 12 + 4 + v) * 64 + lane] = acc16b[v];
        cimg[((wave - 1) * 12 + 8 + v) * 64 + lane] = acc16c[v];
      }
    }
    __syncthreads();
    if (wave != 0) return;
    const int rr = (lane >> 4) * 4, cc = lane & 15;
#pragma unroll
    for (int blk = 0; blk < 3; ++blk) {
      const int bi = blk ? 1 : 0, bj = blk == 2 ? 1 : 0;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float t = blk == 0 ? acc16[v] : blk == 1 ? acc16b[v] : acc16c[v];
#pragma unroll
        for (int w = 0; w < 3; ++w) t += cimg[(w * 12 + blk * 4 + v) * 64 + lane];
        float* at = &out[(16 * bi + rr + v) * TILE + 16 * bj + cc];
        if (!J.accum) *at = t;
        else *at = J.sbeta == 0.f ? J.alpha * t : fmaf(J.sbeta, *at, J.alpha * t);
      }
    }
    return;
  }
  if (mode == 2) {  // sum the 4 waves' 16x16 partials in wave order (deterministic)
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int v = 0; v < 4; ++v) cimg[((wave - 1) * 4 + v) * 64 + lane] = acc16[v];
    }
    __syncthreads();
    if (wave != 0) return;
    // C/D map of 16x16x4: row = (lane >> 4) * 4 + v, col = lane & 15
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      float t = acc16[v];
#pragma unroll
      for (int w = 0; w < 3; ++w) t += cimg[(w * 4 + v) * 64 + lane];
      float* at = &out[((lane >> 4) * 4 + v) * TILE + (lane & 15)];
      if (!J.accum) *at = t;
      else *at = J.sbeta == 0.f ? J.alpha * t : fmaf(J.sbeta, *at, J.alpha * t);
    }
    return;
  }
  // block (bi, bj) = quadrant (bi & 1, bj & 1) of slab tile (bi / 2, bj / 2)
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    if (i >= nmine) break;
    const int bi = bij[i] >> 16, bj = bij[i] & 0xffff, ti = bi >> 1, tj = bj >> 1;
    float* o = J.slab + ((size_t)(ti * (ti + 1) / 2 + tj) * J.sstride + split) * TILE * TILE +
               (bi & 1) * 32 * TILE + (bj & 1) * 32;
    put_partial(J, acc[i], [&](int v) { return &o[acc_row(v, lane) * TILE + (lane & 31)]; });
  }
}

// ------------------------------------------------------------------- host side
// Geometry of a conv job on the LDS-staged kernel; false: the job takes the
// register-staged path (images too large, channel blocks not float4-shaped).
bool conv_fp32_geom(const kfac_operand& o, ConvGeom& g) {
  const int n = g.n;
  g.mode = n <= 16 ? CONV_N16 : (n <= 32 ? CONV_N32 : CONV_BLOCKS);
  g.KR = g.mode != CONV_BLOCKS ? 4 : 2;
  int64_t lds;
  // Bank-conflict-free operand reads: an MFMA's 32 lanes of one lane group read 32
  // consecutive factor columns, column (c, ki, kj) at c*plane + ki*Wp + kj (PATCH) or
  // c*plane (CHANNEL) plus a lane-uniform offset.  ds_read_b32 banks are
  // (addr / 4) mod 32, so with Wp = kw and plane = kh*kw (PATCH) or plane = 1
  // (CHANNEL) modulo 32 every lane hits the bank of its own column index.  (16x16x4
  // CHANNEL blocks put two k-lanes in a group: their segments are 16 apart mod 32.)
  auto pad_to = [](int64_t v, int64_t r) { return v + (((r - v) % 32) + 32) % 32; };
  if (o.layout == KFAC_PATCH) {
    if ((int64_t)o.C * o.H * o.W > CONV_SRC_MAX) return false;
    g.Wp = o.W + 2 * o.pw;
    g.plane = (o.H + 2 * o.ph) * g.Wp;
    if (g.mode != CONV_N16) {  // (CONV_N32 too: its 16-lane groups read 16 consecutive columns)
      const int64_t Wp = pad_to(g.Wp, o.kw);
      const int64_t plane = pad_to((int64_t)(o.H + 2 * o.ph) * Wp, (int64_t)o.kh * o.kw);
      const int64_t need = o.C * plane + 2 * (int64_t)o.Ho * o.sh * Wp;
      if (need <= CONV_LDS_MAX) {
        g.Wp = (int)Wp;
        g.plane = (int)plane;
      }
    }
    g.Ho = o.Ho;
    g.rowstep = o.sh * g.Wp;
    g.T = o.Wo;
    g.G = (int)cdiv(o.Ho, g.KR);
    g.stride = o.sw;
    g.ones_base = o.C * g.plane;  // (= n - 1 mod 32: the bias column's own bank)
    // the padding columns of the last block all read the zero plane (one broadcast
    // address): put it on bank n mod 32, which no data column of that block uses
    // (at its unpadded place it shared a bank with one: 2-way conflicts)
    g.zero_base = g.ones_base + o.Ho * g.rowstep;
    g.zero_base += (int)((((int64_t)n - g.zero_base) % 32 + 32) % 32);
    lds = (int64_t)g.zero_base + o.Ho * g.rowstep;
    g.src = o.C * o.H * o.W;
  } else {
    const int64_t img = (int64_t)o.cols * o.L;
    if (o.L % 4 != 0 || o.sB % 4 != 0 || reinterpret_cast<uintptr_t>(o.ptr) % 16 != 0 ||
        img / 4 > CONV_SRC_MAX)
      return false;
    // (a multi-batch job's other batch bases: the router checks their alignment)
    const int segs = g.mode != CONV_BLOCKS ? 4 * g.KR : g.KR;  // narrow: the 4 waves' segments too
    int Q = (int)cdiv(o.L, segs);
    if (g.mode != CONV_BLOCKS) Q = (int)pad_to(Q, 16);
    g.rowstep = Q;
    g.plane = (int)pad_to((int64_t)segs * Q, 1);
    g.T = Q;
    g.G = 1;
    g.stride = 1;
    g.Ho = 1;
    g.zero_base = g.ones_base = o.cols * g.plane;
    lds = (int64_t)g.zero_base + g.plane;
    g.src = (int)(img / 4);
  }
  lds = std::max<int64_t>(lds, 3 * 16 * 64);
  if (lds > CONV_LDS_MAX) return false;
  const int nb = (int)cdiv(n, 32);
  g.nq = nb * (nb + 1) / 2;
  g.units = g.mode != CONV_BLOCKS ? 1 : (int)cdiv(g.nq, 4 * CONV_CB);
  g.lds = (int)lds;
  return true;
}

template <int LAYOUT>
static void launch_conv_layout(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream) {
  const size_t shmem = (size_t)g.lds * sizeof(float);
  const bool s1 = g.stride == 1;
  const int pm = (int)cdiv(g.src, NTHREADS);  // <= 8 by CONV_SRC_MAX
  // one instance per mode class, so each gets its own register budget: CONV_BLOCKS (CB
  // blocks per wave), the one-block CONV_N16 (CB = 1), CONV_N32
#define KFAC_CONV_LAUNCH(PM, S1, CBV, M3) \
  hipLaunchKernelGGL((kfac_factor_conv<LAYOUT, PM, S1, CBV, M3>), dim3(tasks), dim3(NTHREADS), shmem, stream, \
                     args, g)
#define KFAC_CONV_PICK(CBV, M3)                                                   \
  do {                                                                            \
    if (pm <= 4) {                                                                \
      if (s1) KFAC_CONV_LAUNCH(4, true, CBV, M3); else KFAC_CONV_LAUNCH(4, false, CBV, M3); \
    } else {                                                                      \
      if (s1) KFAC_CONV_LAUNCH(8, true, CBV, M3); else KFAC_CONV_LAUNCH(8, false, CBV, M3); \
    }                                                                             \
  } while (0)
  if (g.mode == CONV_N32)
    KFAC_CONV_PICK(CONV_CB, true);
  else if (g.mode != CONV_BLOCKS)
    KFAC_CONV_PICK(1, false);
  else
    KFAC_CONV_PICK(CONV_CB, false);
#undef KFAC_CONV_PICK
#undef KFAC_CONV_LAUNCH
}

// (at most 48 KB of dynamic LDS: inside the default limit, no attribute to raise)
int launch_conv(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream) {
  if (args.job[0].x.layout == KFAC_CHANNEL)
    launch_conv_layout<KFAC_CHANNEL>(args, g, tasks, stream);
  else
    launch_conv_layout<KFAC_PATCH>(args, g, tasks, stream);
  return KFAC_OK;
}

}  // namespace kfac
