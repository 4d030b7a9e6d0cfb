#include <algorithm>
#include <array>
#include <cstddef>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <utility>
#include <vector>

#include "bf16x3.h"
#include "factor_common.h"

namespace kfac {

// ------------------------- conv factors from flattened column copies (kfac_factor_conv_x3f)
// The im2col factor of a stride-1 conv layer with 32 < n <= 160 (LeNet-5's conv2 A: 151
// features over 100 positions per image, curvatures.py:341-343) without an im2col.
// With the output positions flattened, p = oh Wo + ow, the patch entry of feature
// (c, ki, kj) at p is padded[c][oh + ki][ow + kj] = copy(c, kj)[ki Wo + p], where
//   copy(c, kj)[r Wo + ow] = padded[c][r][ow + kj]      (r < Hp, ow < Wo)
// is the padded image's column window of width Wo, rows kept at pitch Wo.  So C x kw
// copies (kh x fewer entries than the im2col, 25 KB per LeNet-5 image in three bf16
// parts instead of 102 KB) hold every MFMA fragment -- 8 consecutive positions of one
// feature -- at element ki Wo + p.  8-byte reads need ki Wo + shift = 0 mod 4: each copy
// is kept in NV <= 2 variants shifted by the residues the kernel rows need (LeNet-5
// conv2, Wo = 10: shifts 0 and 2).  Positions past L in the last 16-position k-step
// read the next rows' data, so that k-step's fragments are masked.  The bias row reads
// a ones copy, padding rows a zero copy.
// Copy placement (host, conv_x3f_geom): every copy (c, kj, v) has its own base, chosen so
// the 8-byte fragment reads of each 16-lane group hit 16 distinct bank pairs (a search
// over the bases' residues mod 128 B; a uniform copy stride left 2-way conflicts on 8 of
// LeNet-5's 10 groups: the reads took twice their time, `profiles/r06z4/`).  The bases
// sit in an LDS table (xf_cb, 16 entries per channel).
// As in kfac_factor_conv_x3s: one workgroup of 8 waves per CU, two copy buffers, two groups of 4
// waves that swap roles every image (one multiplies image i, the other builds image
// i + 1 and loads image i + 3).  The build works from per-slot records made once per
// task (source offsets, destination offset, kernel columns in range): recomputing the
// slot geometry per image (integer divisions) and a branch per copy made the build the
// bound (3.9 us per image against 3.6 us of MFMAs; 425 VALU, 104 branches per wave).
constexpr int XF_THREADS = 512;
constexpr int XF_WAVES = XF_THREADS / 64;
constexpr int XF_GROUP = XF_THREADS / 2;  // threads per role group
constexpr int XF_GW = XF_WAVES / 2;       // waves per role group
constexpr int XF_SP = 3;                  // build slots per group thread and image (<= 768)
constexpr int XF_BPW = 4;                 // blocks per multiplying wave (nq <= 16)
constexpr int XF_KW = 8;                  // kernel width at most
constexpr int XF_CB = 256;                // copy-base table entries (C x 2 XF_KW: C <= 16)
constexpr int XF_PART = 19456;            // bytes per part (copies, ones, zero, dummy)
constexpr int XF_BUF = 3 * XF_PART;       // one copy buffer (hi, mid, lo parts)
constexpr int XF_REC = 2 * XF_BUF;        // build-slot records: [slot i][group thread] u32x2
constexpr int XF_TBL = XF_REC + XF_SP * XF_GROUP * 8;  // copy bases: u16 [c][kj][v] (v < 2)
constexpr int XF_LDS = XF_TBL + XF_CB * 2;  // (a 29 KB inversion workgroup still fits beside it)
static_assert(XF_LDS <= 134144, "x3f LDS");

// A multiplying wave's blocks as pairs (a, b) of indices into its fragment set F: block
// (F[a], F[b]); a diagonal block (a = b) takes x3_four (four MFMAs and a transposed
// half, acc2) instead of six.  Assignments (conv_x3f_geom), from an exact-cover search
// over the lower triangle's blocks (<= 4 blocks and <= 4 fragments per wave, block order
// maximizing the MFMAs between a fragment's reload and its next use):
//   5 block rows (n = 129..160): F = {0,1,2,3} (0,0) (1,1) (3,2) -- 14 MFMAs per k-step;
//     {0,1,2,4} (2,2) (2,0) (1,0) (4,1); {1,2,3,4} (2,1) (3,1) (4,3) (4,4);
//     {0,2,3,4} (3,3) (3,0) (4,0) (4,2) -- 22 each (six-product diagonals: 24 on the
//     busiest wave), >= 8 MFMAs of slack per reload (was 6);
//   4 block rows (97..128): F = {0,1,2,3} for all: (0,0) (1,1) (3,2); (1,0) (2,2) (3,3);
//     (2,0) (3,1); (2,1) (3,0) -- 14, 14, 12, 12.
struct XfPat {
  int a[4], b[4], n;
};
constexpr XfPat XF_PAT[] = {
    {{0, 1, 3, 0}, {0, 1, 2, 0}, 3}, {{2, 2, 1, 3}, {2, 0, 0, 1}, 4}, {{1, 2, 3, 3}, {0, 0, 2, 3}, 4},
    {{2, 2, 3, 3}, {2, 0, 0, 1}, 4}, {{1, 2, 3, 0}, {0, 2, 3, 0}, 3}, {{2, 3, 0, 0}, {0, 1, 0, 0}, 2},
    {{2, 3, 0, 0}, {1, 0, 0, 0}, 2}};
constexpr int XF_NPAT = sizeof(XF_PAT) / sizeof(XF_PAT[0]);
constexpr int XF_D2 = 2;  // diagonal blocks per wave at most (acc2 sets)
// (the epilogue's exchange -- 4 waves x 6 sets of 16 x 64 floats -- and 4 transpose tiles
// fit the two copy buffers)
static_assert(2 * XF_BUF >= (XF_GW * (XF_BPW + XF_D2) * 16 * 64 + XF_GW * 32 * 33) * 4, "x3f epilogue LDS");
__host__ __device__ constexpr int xf_pat_frags(const XfPat& p) {
  int m = 0;
  for (int s = 0; s < p.n; ++s) m = std::max(m, std::max(p.a[s], p.b[s]) + 1);
  return m;
}
__host__ __device__ constexpr int xf_pat_last_use(const XfPat& p, int q) {
  int l = -1;
  for (int s = 0; s < p.n; ++s)
    if (p.a[s] == q || p.b[s] == q) l = s;
  return l;
}
__host__ __device__ constexpr int xf_pat_diag(const XfPat& p, int s) {  // acc2 set of block s
  int d = 0;
  for (int t = 0; t < s; ++t) d += p.a[t] == p.b[t];
  return d;
}
__host__ __device__ inline int xf_pat_blocks(int pat) { return XF_PAT[pat].n; }
__host__ __device__ inline int xf_pat_a(int pat, int s) { return XF_PAT[pat].a[s]; }
__host__ __device__ inline int xf_pat_b(int pat, int s) { return XF_PAT[pat].b[s]; }

// The kernel reads cg.xf_cb through the kernel-argument pointer, at the offset where the
// second argument follows the first (its `cgo`): the table must lie inside that argument.
// The sizes are pinned because every factor kernel takes these structs by value: with
// the 256 B of implicit arguments, 4,744 B of kernel arguments for the FactorArgs kernels
// and 5,608 B with a ConvGeom.
constexpr size_t XF_CGO = (sizeof(FactorArgs) + alignof(ConvGeom) - 1) / alignof(ConvGeom) * alignof(ConvGeom);
static_assert(XF_CGO + offsetof(ConvGeom, xf_cb) + XF_CB * 2 <= XF_CGO + sizeof(ConvGeom),
              "x3f copy-base table inside the ConvGeom kernel argument");
static_assert(sizeof(FactorArgs) == 4488 && XF_CGO + sizeof(ConvGeom) == 5352, "kernel-argument layout");

__global__ __launch_bounds__(XF_THREADS, 1) void kfac_factor_conv_x3f(FactorArgs args, ConvGeom cg) {
  extern __shared__ __attribute__((aligned(16))) char cxf[];
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int jx = 0;
  while (jx + 1 < args.njobs && task >= args.task_end[jx]) ++jx;
  const FactorJobDev& J = args.job[jx];
  const OpDev& op = J.x;
  const int split = task - J.task_begin;  // one unit: task = split
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t b0 = (int64_t)split * cg.B / J.splits, b1 = (int64_t)(split + 1) * cg.B / J.splits;
  const int gt = tid % XF_GROUP, grp = wave / XF_GW;
  const int nsp = (cg.xs_np + XF_GROUP - 1) / XF_GROUP;
  u32x2* rec = reinterpret_cast<u32x2*>(cxf + XF_REC);
  uint16_t* tbl = reinterpret_cast<uint16_t*>(cxf + XF_TBL);
  // once per task: zero both buffers; the copy-base table from the kernel argument
  // (constant-index reads: a lane-indexed read of the argument copies it to scratch)
  for (int e = tid; e < 2 * XF_BUF / 16; e += XF_THREADS) reinterpret_cast<u32x4*>(cxf)[e] = u32x4{0u, 0u, 0u, 0u};
  if (tid < XF_CB / 2) {
    // (read through the kernel-argument pointer: cg is the second argument, at its
    // alignment after FactorArgs)
    typedef const __attribute__((address_space(4))) char kchar;
    typedef const __attribute__((address_space(4))) int kint;
    kchar* ka = (kchar*)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr size_t cgo = (sizeof(FactorArgs) + alignof(ConvGeom) - 1) / alignof(ConvGeom) * alignof(ConvGeom);
    reinterpret_cast<int*>(tbl)[tid] = ((kint*)(ka + cgo + offsetof(ConvGeom, xf_cb)))[tid];
  }
  // the build-slot records (c, r, col): col even in padded coordinates; elements col ..
  // col + 2 of padded row r of channel c, their pairs written to copy (c, kj) at
  // ow = col - kj (kj even) or col + 1 - kj (kj odd), 0 <= ow < Wo (Wo even: a pair is
  // wholly in or out).  x: source dword + 8 (bits 0-15), elements in the image (bits
  // 16-18); y: 2 (r Wo + col) (bits 0-15), c (16-23), kernel columns in range (24-31)
  const int wp2 = cg.xs_wp2, rowp = cg.xs_hp * wp2;
  if (tid < XF_GROUP)
    for (int i = 0; i < nsp; ++i) {
      const int e = tid + i * XF_GROUP;
      uint32_t x = 0, y = 0;
      if (e < cg.xs_np) {
        const int c = e / rowp, rem = e - c * rowp, r = rem / wp2, col = 2 * (rem - r * wp2);
        const int h = r - op.ph;
        uint32_t dm = 0, km = 0;
        for (int d = 0; d < 3; ++d) {
          const int w = col + d - op.pw;
          if (h >= 0 && h < op.H && w >= 0 && w < op.W) dm |= 1u << d;
        }
        for (int kj = 0; kj < op.kw; ++kj) {
          const int ow = col - kj + (kj & 1);
          if (ow >= 0 && ow < cg.Wo) km |= 1u << kj;
        }
        x = (uint32_t)(dm ? (c * op.H + h) * op.W + col - op.pw + 8 : 0) | dm << 16;
        y = (uint32_t)(2 * (r * cg.Wo + col)) | (uint32_t)c << 16 | km << 24;
      }
      rec[i * XF_GROUP + tid] = u32x2{x, y};
    }
  __syncthreads();
  if (cg.ones >= 0)
    for (int e = tid; e < 2 * cg.L; e += XF_THREADS) {
      const int bs = e / cg.L, p = e - bs * cg.L;
      *reinterpret_cast<uint16_t*>(cxf + bs * XF_BUF + cg.xf_one + 2 * p) = 0x3f80;
    }
  constexpr int OUT = 0x7ffffff0;
  const int irec = op.C * op.H * op.W * 4;  // bytes of one image
  float v0[XF_SP][3];
  auto fetch = [&](int64_t b, const u32x2 (&rc)[XF_SP]) __attribute__((always_inline)) {
    const int seg = (int)((uint32_t)b / (uint32_t)cg.bseg);
    const float* src = seg_base(J, args.segs, seg) + (b - (int64_t)seg * cg.bseg) * op.sB;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(src), 0, irec, 0x00020000);
#pragma unroll
    for (int i = 0; i < XF_SP; ++i) {
      if (i >= nsp) break;
      const int s0 = (int)(rc[i].x & 0xffffu) * 4 - 32;
#pragma unroll
      for (int d = 0; d < 3; ++d)
        v0[i][d] = __uint_as_float(
            __builtin_amdgcn_raw_buffer_load_b32(rs, (rc[i].x >> (16 + d)) & 1u ? s0 + 4 * d : OUT, 0, 0));
    }
  };
  auto records = [&](u32x2 (&rc)[XF_SP]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < XF_SP; ++i) rc[i] = i < nsp ? rec[i * XF_GROUP + gt] : u32x2{0u, 0u};
  };
  // out-of-range kernel columns write to a dummy row (one dword per lane) instead of a
  // branch per copy
  const int NV = cg.xf_nv, KW = op.kw;
  const int dummy = cg.xf_dummy + 4 * lane;
  auto build = [&](char* buf, const u32x2 (&rc)[XF_SP]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < XF_SP; ++i) {
      if (i >= nsp) break;
      uint32_t p0[3], p1[3];
      split3(v0[i][0], v0[i][1], p0[0], p0[1], p0[2]);
      split3(v0[i][1], v0[i][2], p1[0], p1[1], p1[2]);
      const int q = (int)(rc[i].y & 0xffffu), c = (int)((rc[i].y >> 16) & 0xffu);
      const uint32_t km = rc[i].y >> 24;
      const u32x4* tb = reinterpret_cast<const u32x4*>(tbl + c * 2 * XF_KW);
      const u32x4 t0 = tb[0], t1 = tb[1];  // this channel's copy bases, [kj][v]
#pragma unroll
      for (int kj = 0; kj < XF_KW; ++kj) {
        if (kj >= KW) break;
        const uint32_t wv = kj < 4 ? t0[kj] : t1[kj - 4];
        const bool in = (km >> kj) & 1u;
        const int qk = q + 2 * ((kj & 1) - kj);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          if (v >= NV) break;
          const int base = (int)(v ? wv >> 16 : wv & 0xffffu);
          char* d = buf + (in ? base + qk : dummy);
#pragma unroll
          for (int r = 0; r < 3; ++r)
            *reinterpret_cast<uint32_t*>(d + r * XF_PART) = (kj & 1) ? p1[r] : p0[r];
        }
      }
    }
  };
  // this wave's fragment set F (<= 4 block rows of the factor: A of block (bi, bj) is
  // fragment bi, B fragment bj -- one matrix) and its blocks as pairs of F indices, from
  // a fixed menu of patterns (XF_PAT), so one k-step reads |F| fragments for up to 4
  // blocks (LeNet-5's conv2: 14 fragment reads per k-step for 15 blocks instead of 30;
  // at two 8-byte reads per fragment and part the LDS was the bound)
  const int gw = wave % XF_GW, m = lane & 31, hh = lane >> 5;
  auto row_off = [&](int f) __attribute__((always_inline)) {
    if (f < op.cols) {
      const int kk = op.kh * op.kw, c = f / kk, rr = f - c * kk, ki = rr / op.kw, kj = rr - ki * op.kw;
      const int v = (cg.xf_vmap >> (2 * ki)) & 3;
      return (int)tbl[c * 2 * XF_KW + 2 * kj + v] + 2 * ki * cg.Wo;
    }
    return f == cg.ones ? cg.xf_one : cg.xf_zero;
  };
  int wcode = 0;  // (constant-index reads of the argument: see mode 5)
#pragma unroll
  for (int t = 0; t < XF_GW; ++t) {
    int e = cg.xf_wave[t];
    asm volatile("" : "+s"(e));
    wcode = gw == t ? e : wcode;
  }
  const int pat = wcode & 15;  // bits 4 + 3 q .. : F[q]
  int offF[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) offF[q] = row_off(32 * ((wcode >> (4 + 3 * q)) & 7) + m) + 16 * hh;
  floatx16 acc[XF_BPW], acc2[XF_D2];
#pragma unroll
  for (int i = 0; i < XF_BPW; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;
#pragma unroll
  for (int i = 0; i < XF_D2; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc2[i][v] = 0.f;
  // the last k-step's positions past L (L even): fragments masked by dword
  const int nks = cg.xf_nks, last = nks - 1;
  const int vc = min(max(cg.L - (16 * last + 8 * hh), 0), 8);
  uint32_t amask[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) amask[d] = 2 * d + 1 < vc ? 0xffffffffu : 0u;
  auto rd8 = [&](const char* p) __attribute__((always_inline)) {  // 8 bf16 from two 8-byte reads
    const u32x2 lo = *reinterpret_cast<const u32x2*>(p), hi2 = *reinterpret_cast<const u32x2*>(p + 8);
    return __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi2.x, hi2.y});
  };
  auto mask_all = [&](X3Frag* F, int nf) __attribute__((always_inline)) {  // (in place)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q >= nf) break;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        u32x4 w = __builtin_bit_cast(u32x4, F[q].p[r]);
#pragma unroll
        for (int d = 0; d < 4; ++d) w[d] &= amask[d];
        F[q].p[r] = __builtin_bit_cast(bf16x8, w);
      }
    }
  };
  // one register set: after the block that uses a fragment last in this k-step, the
  // fragment is reloaded for the next one, so each load has the following blocks'
  // MFMAs to land (two whole sets of 4 fragments left no registers for the rest:
  // spills).  The block orders of XF_PAT put a fragment's last use before the next
  // k-step's first use wherever the pattern allows.  The last k-step's fragments are
  // masked in place (a zero A or B element zeroes the product).
  auto mma_pat = [&](const char* buf, auto PI) __attribute__((always_inline)) {
    constexpr XfPat P = XF_PAT[decltype(PI)::value];
    constexpr int NF = xf_pat_frags(P);
    X3Frag F[NF];
    auto load = [&](int t, int q) __attribute__((always_inline)) {
#pragma unroll
      for (int r = 0; r < 3; ++r) F[q].p[r] = rd8(buf + r * XF_PART + offF[q] + 32 * t);
    };
    // (first reads in the loop's order -- by last use -- so the wait at the loop head
    // holds for the entry as for the back edge; in fragment order it was lgkmcnt(0);
    // the last k-step peeled: a mask at the loop head made every k-step wait for all
    // of its reads)
#pragma unroll
    for (int s2 = 0; s2 < P.n; ++s2)
#pragma unroll
      for (int q = 0; q < NF; ++q)
        if (xf_pat_last_use(P, q) == s2) load(0, q);
    auto prod = [&](int s2) __attribute__((always_inline)) {  // (s2: unrolled constant)
      if (P.a[s2] == P.b[s2]) x3_four(acc[s2], acc2[xf_pat_diag(P, s2)], F[P.a[s2]]);
      else x3_six(acc[s2], F[P.a[s2]], F[P.b[s2]]);
    };
    for (int t = 0; t < last; ++t) {
#pragma unroll
      for (int s2 = 0; s2 < P.n; ++s2) {
        prod(s2);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NF; ++q)
          if (xf_pat_last_use(P, q) == s2) load(t + 1, q);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    mask_all(F, NF);
#pragma unroll
    for (int s2 = 0; s2 < P.n; ++s2) prod(s2);
  };
  auto mma = [&](const char* buf) __attribute__((always_inline)) {
    switch (pat) {
      case 0: mma_pat(buf, std::integral_constant<int, 0>{}); break;
      case 1: mma_pat(buf, std::integral_constant<int, 1>{}); break;
      case 2: mma_pat(buf, std::integral_constant<int, 2>{}); break;
      case 3: mma_pat(buf, std::integral_constant<int, 3>{}); break;
      case 4: mma_pat(buf, std::integral_constant<int, 4>{}); break;
      case 5: mma_pat(buf, std::integral_constant<int, 5>{}); break;
      case 6: mma_pat(buf, std::integral_constant<int, 6>{}); break;
      default: break;
    }
  };
  // phases as mode 5: group i % 2 multiplies image i, the other builds image i + 1 and
  // loads image i + 3; one straight-line loop per group
  const int64_t nimg = b1 - b0;
  auto phase_mma = [&](int64_t i) __attribute__((always_inline)) {
    if (i < nimg) mma(cxf + (int)(i & 1) * XF_BUF);
    __syncthreads();
  };
  auto phase_build = [&](int64_t i) __attribute__((always_inline)) {
    if (i + 1 < nimg) {
      u32x2 rc[XF_SP];
      records(rc);
      build(cxf + (int)((i + 1) & 1) * XF_BUF, rc);
      if (i + 3 < nimg) fetch(b0 + i + 3, rc);
    }
    __syncthreads();
  };
  if (grp == 0) {
    if (nimg > 0) {
      u32x2 rc[XF_SP];
      records(rc);
      fetch(b0, rc);
      build(cxf, rc);
      if (nimg > 2) {
        fetch(b0 + 2, rc);
#pragma unroll
        for (int i = 0; i < XF_SP; ++i) asm volatile("" ::"v"(v0[i][0]), "v"(v0[i][1]), "v"(v0[i][2]));  // (landed)
      }
    }
    __syncthreads();
    for (int64_t i = 0; i < nimg; i += 2) {
      phase_mma(i);
      phase_build(i + 1);
    }
  } else {
    if (nimg > 1) {
      u32x2 rc[XF_SP];
      records(rc);
      fetch(b0 + 1, rc);
    }
    __syncthreads();
    for (int64_t i = 0; i < nimg; i += 2) {
      phase_build(i);
      phase_mma(i + 1);
    }
  }
  // group 1's partial sums added to group 0's (fixed order), then the diagonal blocks'
  // acc + acc2 + acc2^T (the transpose through a per-wave LDS tile: a wave's LDS
  // operations complete in order), stored by group 0 (its accumulator reads in flight
  // across the exchange)
  float* red = reinterpret_cast<float*>(cxf);
  constexpr int XF_SETS = XF_BPW + XF_D2;
  const int nblk = pat < XF_NPAT ? xf_pat_blocks(pat) : 0;
  auto at = [&](int i, int v) __attribute__((always_inline)) {
    const int bi = (wcode >> (4 + 3 * xf_pat_a(pat, i))) & 7, bj = (wcode >> (4 + 3 * xf_pat_b(pat, i))) & 7;
    const int ti = bi >> 1, tj = bj >> 1;
    float* o = J.slab + ((size_t)(ti * (ti + 1) / 2 + tj) * J.sstride + split) * TILE * TILE +
               (bi & 1) * 32 * TILE + (bj & 1) * 32;
    return &o[acc_row(v, lane) * TILE + (lane & 31)];
  };
  float old[XF_BPW][16];
  if (grp == 1) {
#pragma unroll
    for (int i = 0; i < XF_SETS; ++i)
#pragma unroll
      for (int v = 0; v < 16; ++v)
        red[((gw * XF_SETS + i) * 16 + v) * 64 + lane] = i < XF_BPW ? acc[i][v] : acc2[i - XF_BPW][v];
  } else {
    load_partials(J, nblk, old, at);
  }
  __syncthreads();
  if (grp == 1) return;
#pragma unroll
  for (int i = 0; i < XF_BPW; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[i][v] += red[((gw * XF_SETS + i) * 16 + v) * 64 + lane];
#pragma unroll
  for (int i = 0; i < XF_D2; ++i)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc2[i][v] += red[((gw * XF_SETS + XF_BPW + i) * 16 + v) * 64 + lane];
  float* tr = red + XF_GW * XF_SETS * 16 * 64 + gw * 32 * 33;  // this wave's 32 x 33 tile
  int d = 0;
#pragma unroll
  for (int i = 0; i < XF_BPW; ++i) {
    if (i >= nblk) break;
    if (xf_pat_a(pat, i) != xf_pat_b(pat, i)) continue;
    floatx16 y = acc2[0];
#pragma unroll
    for (int v = 0; v < 16; ++v) y[v] = d ? acc2[1][v] : y[v];
#pragma unroll
    for (int v = 0; v < 16; ++v) tr[acc_row(v, lane) * 33 + (lane & 31)] = y[v];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[i][v] += y[v] + tr[(lane & 31) * 33 + acc_row(v, lane)];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the tile's reads before its next writes)
    ++d;
  }
  put_partials(J, nblk, acc, old, at);
}

// ------------------------------------------------------------------- host side
// x3f_search: a stride-1 im2col operand with 32 < n <= 160 (<= 16
// blocks: 4 per multiplying wave), even Wo (bf16 pairs), kernel <= 8 x 8, C <= 16, whose
// copies fit in XF_PART and take at most XF_SP build slots per thread.
// Copy bases: the fragment row of feature (c, ki, kj) starts at 8-byte unit
// base(c, kj, v(ki)) + (ki Wo + shift) / 4; a 16-lane group of ds_read_b64 / ds_read2_b64
// is conflict-free when its 16 distinct units are distinct mod 16 (equal addresses
// broadcast: the zero rows).  A depth-first search over the copies' residues mod 16
// (in order of first use, <= 2^20 nodes) finds such bases (LeNet-5's conv2: 15 k nodes),
// then the copies are laid out in a chain that keeps the gaps between them small.
static bool xf_place(const kfac_operand& o, int nb, int nv, int vmap, const int* sft, int zo, int* res) {
  const int ncp = o.C * o.kw * nv, nc = ncp + 1;  // + the ones / zero region
  const int ones = o.has_ones ? o.cols : -1, ng = 2 * nb;
  auto feat = [&](int f, int& cp, int& off) {
    if (f < o.cols) {
      const int kk = o.kh * o.kw, c = f / kk, rr = f - c * kk, ki = rr / o.kw, kj = rr - ki * o.kw;
      const int v = (vmap >> (2 * ki)) & 3;
      cp = (c * o.kw + kj) * nv + v;
      off = (ki * o.Wo + sft[v]) / 4;
    } else {
      cp = ncp;
      off = f == ones ? 0 : zo;
    }
  };
  // uses[cp]: (group, offset) pairs, distinct
  std::vector<std::vector<std::pair<int, int>>> uses(nc);
  std::vector<int> first(nc, 1 << 30);
  for (int g = 0; g < ng; ++g)
    for (int f = 16 * g; f < 16 * g + 16; ++f) {
      int cp, off;
      feat(f, cp, off);
      bool dup = false;
      for (auto& u : uses[cp]) dup |= u.first == g && u.second == off;
      if (!dup) uses[cp].push_back({g, off});
      first[cp] = std::min(first[cp], g);
    }
  std::vector<int> order(nc);
  for (int i = 0; i < nc; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return first[x] < first[y]; });
  std::vector<uint16_t> used(ng, 0);
  int64_t nodes = 0;
  std::function<bool(int)> dfs = [&](int k) -> bool {
    if (k == nc) return true;
    if (++nodes > (1 << 20)) return false;
    const int i = order[k];
    for (int r = 0; r < 16; ++r) {
      bool ok = true;
      for (auto& u : uses[i]) ok &= !((used[u.first] >> ((r + u.second) & 15)) & 1);
      if (!ok) continue;
      for (auto& u : uses[i]) used[u.first] |= (uint16_t)(1u << ((r + u.second) & 15));
      res[i] = r;
      if (dfs(k + 1)) return true;
      for (auto& u : uses[i]) used[u.first] &= (uint16_t)~(1u << ((r + u.second) & 15));
    }
    return false;
  };
  return dfs(0);
}

static bool x3f_search(const kfac_operand& o, ConvGeom& g) {
  const int n = g.n;
  if (n <= 32 || o.sh != 1 || o.sw != 1 || o.Ho <= 0 || o.Wo <= 0 || o.Wo % 2 != 0 || o.kw > XF_KW ||
      o.kh > 8 || o.C > XF_CB / (2 * XF_KW) || (int64_t)o.C * o.H * o.W + 16 > 0xffff)
    return false;
  const int nb = (int)cdiv(n, 32), nq = nb * (nb + 1) / 2;
  if (nb != 4 && nb != 5) return false;  // (the fragment-sharing assignments, XF_PAT)
  const int hp = o.H + 2 * o.ph, wp2 = (o.W + 2 * o.pw + 1) / 2;
  const int64_t np = (int64_t)o.C * hp * wp2;
  if (np > (int64_t)XF_SP * XF_GROUP || 2 * (hp * o.Wo + 2 * wp2) > 0xffff) return false;
  // the shifts that align ki Wo + shift to 4 elements, one variant per distinct shift
  int nv = 0, vmap = 0, shifts[4];
  for (int ki = 0; ki < o.kh; ++ki) {
    const int sft = (4 - (ki * o.Wo) % 4) % 4;
    int v = 0;
    while (v < nv && shifts[v] != sft) ++v;
    if (v == nv) shifts[nv++] = sft;
    vmap |= v << (2 * ki);
  }
  if (nv > 2) return false;  // (the build writes two variants at most)
  const int ncp = o.C * o.kw * nv;
  const int nks = (int)cdiv(o.L, 16);
  const int cu = (hp * o.Wo + 3 + 3) / 4;  // 8-byte units per copy (elements shift .. shift + Hp Wo)
  const int zo = 4 * nks + 2;               // the zero copy after the ones copy (units)
  std::vector<int> res(ncp + 1);
  if (!xf_place(o, nb, nv, vmap, shifts, zo, res.data())) return false;
  // chain layout: the next copy is the one whose residue is reached with the least gap
  std::vector<std::vector<int>> pool(16);
  for (int i = ncp - 1; i >= 0; --i) pool[res[i]].push_back(i);
  std::vector<int> base(ncp + 1);
  int p = 0;
  for (int left = ncp; left > 0; --left)
    for (int gap = 0; gap < 16; ++gap) {
      auto& q = pool[(p + gap) & 15];
      if (q.empty()) continue;
      base[q.back()] = p + gap;
      q.pop_back();
      p += gap + cu;
      break;
    }
  while ((p & 15) != res[ncp]) ++p;
  base[ncp] = p;
  // ones copy, zero copy (16 nks + 8 bf16 of reads each), the dummy row (64 dwords, and
  // the last k-step's over-reads past any copy land before the part's end)
  const int dummy = 8 * (p + zo + 4 * nks + 4);
  if (dummy + 256 + 64 > XF_PART) return false;
  g.nb = nb;
  g.nq = nq;
  auto wave_code = [](int pat, std::initializer_list<int> f) {
    int c = pat, q = 0;
    for (int x : f) c |= x << (4 + 3 * q++);
    return c;
  };
  if (nb == 5) {
    g.xf_wave[0] = wave_code(0, {0, 1, 2, 3});
    g.xf_wave[1] = wave_code(1, {0, 1, 2, 4});
    g.xf_wave[2] = wave_code(2, {1, 2, 3, 4});
    g.xf_wave[3] = wave_code(3, {0, 2, 3, 4});
  } else {
    g.xf_wave[0] = wave_code(0, {0, 1, 2, 3});
    g.xf_wave[1] = wave_code(4, {0, 1, 2, 3});
    g.xf_wave[2] = wave_code(5, {0, 1, 2, 3});
    g.xf_wave[3] = wave_code(6, {0, 1, 2, 3});
  }
  g.xs_hp = hp;
  g.xs_wp2 = wp2;
  g.xs_np = (int)np;
  g.xf_nv = nv;
  g.xf_vmap = vmap;
  for (int c = 0; c < o.C; ++c)
    for (int kj = 0; kj < o.kw; ++kj)
      for (int v = 0; v < nv; ++v) {
        const int e = 16 * c + 2 * kj + v, b = 8 * base[(c * o.kw + kj) * nv + v] + 2 * shifts[v];
        g.xf_cb[e / 2] |= b << (16 * (e & 1));
      }
  g.xf_one = 8 * base[ncp];
  g.xf_zero = 8 * (base[ncp] + zo);
  g.xf_dummy = dummy;
  g.L = (int)o.L;
  g.xf_nks = nks;
  g.Wo = o.Wo;
  g.sh = o.sh;
  g.sw = o.sw;
  g.ones = o.has_ones ? o.cols : -1;
  g.ldsb = XF_LDS;
  g.units = 1;
  return true;
}

// x3f_search, memoized per shape (the plan is made per call: uncached, the residue search
// and layout cost 7 ms per LeNet-5 pass)
bool conv_x3f_geom(const kfac_operand& o, ConvGeom& g) {
  typedef std::array<int64_t, 12> Key;
  static std::mutex mu;
  static std::vector<std::pair<Key, std::pair<bool, ConvGeom>>> memo;
  const Key k{o.C, o.H, o.W, o.kh, o.kw, o.ph, o.pw, o.sh, o.sw, o.Ho * 65536 + o.Wo, o.cols * 2 + (o.has_ones ? 1 : 0),
              (int64_t)g.n};
  {
    std::lock_guard<std::mutex> lk(mu);
    for (auto& e : memo)
      if (e.first == k) {
        if (!e.second.first) return false;
        ConvGeom r = e.second.second;
        // (the fields set before this search: kept from the caller)
        r.B = g.B;
        r.bseg = g.bseg;
        g = r;
        return true;
      }
  }
  ConvGeom r = g;
  const bool ok = x3f_search(o, r);
  std::lock_guard<std::mutex> lk(mu);
  if (memo.size() < 64) memo.push_back({k, {ok, r}});
  if (ok) g = r;
  return ok;
}

int launch_conv_x3f(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream) {
  static const int lds = raise_dynamic_lds(reinterpret_cast<const void*>(&kfac_factor_conv_x3f), XF_LDS);
  if (lds != KFAC_OK) return lds;
  hipLaunchKernelGGL(kfac_factor_conv_x3f, dim3(tasks), dim3(XF_THREADS), (size_t)g.ldsb, stream, args, g);
  return KFAC_OK;
}

}  // namespace kfac
