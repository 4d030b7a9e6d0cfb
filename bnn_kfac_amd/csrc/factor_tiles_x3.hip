#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "bf16x3.h"
#include "factor_common.h"

namespace kfac {

// ------------------------------- fp32 operands, bf16x3 products split in registers
// kfac_factor_tiles_x3: TWO waves per work unit, each computing ALL the unit's blocks over
// its own 16-row half of every 32-row stage.  A unit is a clique of up to four 32-column
// panels of the factor (factor_common.h, x3_unit_table): a lane loads its MFMA fragment of
// each panel -- 8 consecutive k of one column -- straight from global memory into
// registers (no LDS), splits it (split3: the exact three-part split of the bf16x3 kernels
// above) and the wave runs six v_mfma_f32_32x32x16_bf16 per 32 x 32 block between two of
// the panels: a K4 unit is 36 MFMAs on 4 splits per wave and 16-row half, where the
// 64 x 64 tile units this kernel had before were 24 on 4 (7.3 split VALU per MFMA: the
// kernel is bound by its issue port, not by the matrix cores).  The two waves' partial
// blocks are summed through LDS in a fixed order at the end.
// Measured on the MNIST MLP group (profiles/r03_x3/ab/probe_summary.txt): direct loads
// beat LDS-DMA rings (shared, one barrier per stage, or one per wave without a
// barrier: 179 vs 196-204 us per 32,768-row launch), the compiled split beats a
// hand-ordered asm one, and 128 x 128 macro tiles with the split made once per macro
// tile into the syrk3 LDS image (x3m) lost (224 us).
constexpr int X3_THREADS = 128;

constexpr int X3_NW = X3_THREADS / 64;

// Operands straight from global memory into registers, no LDS: a lane's fragment is
// rows kw .. kw+7 of one column, eight buffer loads that differ only in their SGPR
// offset (r * ld * 4 bytes), so the addressing costs no VALU; the buffer's record
// limit (the batch's bytes) zero-fills rows past the batch.  The next stage's
// fragments are loaded while the current ones are split and multiplied.
struct X3Col {
  int voff;  // byte offset of (row 16 wave + 8 h, column) from the batch base
  bool fill; // a column past the operand's data (fill value instead)
  float fv;  // its fill value (the ones column: 1)
};

__device__ __forceinline__ void x3_load8(float (&x)[8], __amdgpu_buffer_rsrc_t rs, const X3Col& c,
                                         int sbase, int sstep) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    x[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, c.voff, sbase + r * sstep, 0));
}

// The stage loop: software-pipelined segments in ONE straight-line block.  The fragments
// of the stage's first block -- F0 and F1 -- are split during the previous stage; every
// segment is the six MFMAs of one block interleaved (sched_group_barrier) with the split
// of a fragment a later block needs, and that fragment's registers are reloaded as soon
// as its split has read them:
//   K4:  (1,0) | split F2    (2,0) | split F3    (3,0)
//        (2,1) | split F0'   (3,1)               (3,2) | split F1'
// (F0 and F1 each end before the next stage's is split: four split fragments live)
// so each load goes out one whole stage before its split (x2, x3 hold the next stage,
// x0, x1 the one after) and no register set is copied (2 waves per SIMD at <= 200 VGPRs
// leave an inversion wave room beside them).
// Every load is unconditional: past the task's range the cursor stops (the last stage
// reloads itself), a batch change is a scalar select (the next batch's base fetched a
// stage ahead), columns past the operand load from past the buffer's record limit (0),
// and the ones column (FILL: only the units whose panels hold it) is a select of 1 / 0 by
// row validity.
// Microbench: tools/microbench/x3w_mb.hip; DESIGN.md §3.1c.
struct X3Cursor {  // a stage to load: batch `seg` (base `b`), first row `k`
  const float* b;
  int seg, k;
};

template <int NV>
__device__ __forceinline__ void x3_pattern() {  // 6 MFMAs, NV VALU each, the reloads early
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);       // MFMA
    if (NV > 0) __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);  // VALU
    // (all 8 reloads after the first MFMA: 170 vs 159-166 us, profiles/r04v/)
    if (i < 4) __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);  // VMEM read
  }
}

// The unit kinds the loop is compiled for: a clique of NP = 4, 3 or 2 panels (every block
// (i, j), i > j, between its panel slots; the slots ascend, so slot i is the block's row
// panel), or the diagonal blocks (s, s) of four panel slots.  Accumulators, in order:
//   K4: (1,0) (2,0) (2,1) (3,0) (3,1) (3,2);  K3 and K2: the first 3 / 1 of them;
//   X3_KDIAG: (0,0) (1,1) (2,2) (3,3).
// The mixed kinds (factor_common.h) -- a diagonal block is x3_six(acc, F, F), as in the
// diagonal kind:
//   X3_KS3D3: (3,0) (3,1) (3,2) (0,0) (1,1) (2,2);  X3_KP1D2: (1,0) (0,0) (1,1).
constexpr int X3_KDIAG = 0, X3_KS3D3 = 5, X3_KP1D2 = 6;
constexpr int X3_NACC = 6;  // (a K4's: the LDS hand-off's slots)
__host__ __device__ constexpr int x3_kind_slots(int kind) {
  return kind == X3_KDIAG || kind == X3_KS3D3 ? 4 : kind == X3_KP1D2 ? 2 : kind;
}
__host__ __device__ constexpr int x3_kind_blocks(int kind) {
  return kind == X3_KDIAG ? 4 : kind == X3_KS3D3 ? 6 : kind == X3_KP1D2 ? 3 : kind * (kind - 1) / 2;
}
// (slot of block b's row / column panel, by the accumulator orders above)
struct X3Block {
  int i, j;
};
__host__ __device__ constexpr X3Block x3_kind_block(int kind, int b) {
  constexpr int BI[6] = {1, 2, 2, 3, 3, 3}, BJ[6] = {0, 0, 1, 0, 1, 2};
  if (kind == X3_KDIAG) return {b & 3, b & 3};
  if (kind == X3_KS3D3) return b < 3 ? X3Block{3, b} : X3Block{b - 3, b - 3};
  if (kind == X3_KP1D2) return b == 0 ? X3Block{1, 0} : X3Block{b - 1, b - 1};
  return {BI[b], BJ[b]};
}

template <int KIND, bool FILL>
__device__ __forceinline__ void x3_loop(const FactorJobDev& J, const float* const* segs, const int (&pn)[4],
                                        int64_t s0, int64_t s1, floatx16 (&acc)[x3_kind_blocks(KIND)]) {
  constexpr bool DIAG = KIND == X3_KDIAG;
  constexpr int NP = x3_kind_slots(KIND);
  static_assert(NP >= 2 && NP <= 4, "a unit has two to four panel slots");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ld4 = (int)J.x.ld * 4;
  const int rows = (int)J.x.rows;
  const int rec = rows * ld4;                  // a batch's bytes (planner: < 2^31)
  // (the ragged last batch's: its rows past x.last_rows read as zeros)
  const int rec_last = rec - J.rdelta * ld4;
  const int lr = 16 * wave + 8 * (lane >> 5);  // lane's first row within a stage
  int voff[4];
  bool onesl[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int c = pn[f] * 32 + (lane & 31);
    voff[f] = c < J.x.cols ? lr * ld4 + c * 4 : rec;  // past the operand: the zero tail
    onesl[f] = c == J.x.ones;
  }
  const int ns = (int)(s1 - s0);
  const int lastseg = J.nseg - 1;
  // stage cursors: c1 = the next stage to load for fragments 2 / 3, c2 = the one after
  // (fragments 0 / 1); nb = the base of the batch after c2's
  X3Cursor c2;
  c2.seg = (int)(s0 / J.sps);
  c2.k = (int)((s0 - (int64_t)c2.seg * J.sps) * BK);
  c2.b = seg_base(J, segs, c2.seg);
  const float* nb = seg_base(J, segs, min(c2.seg + 1, lastseg));
  int left = ns - 1;  // stages after c2's within the task (the cursor stops at the last)
  auto advance = [&](X3Cursor& c) {
    const bool more = left > 0;
    const bool wrap = more && c.k + BK >= rows;
    c.k = more ? (wrap ? 0 : c.k + BK) : c.k;
    c.seg += wrap;
    c.b = wrap ? nb : c.b;
    nb = seg_base(J, segs, min(c.seg + 1, lastseg));
    left -= more;
  };
  auto rsrc = [&](const float* b, int seg) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(b), 0, seg == lastseg ? rec_last : rec,
                                             0x00020000);
  };
  auto ld8 = [&](int f, const X3Cursor& c, float (&x)[8]) {
    x3_load8(x, rsrc(c.b, c.seg), X3Col{voff[f], false, 0.f}, c.k * ld4, ld4);
  };
  float x[4][8];
  // prologue: stage s0 into every fragment, the first block's fragments split, their
  // registers reloaded with stage s0 + 1
  const int k0 = c2.k, seg0 = c2.seg;
#pragma unroll
  for (int f = 0; f < NP; ++f) ld8(f, c2, x[f]);
  advance(c2);
  X3Cursor c1 = c2;  // (fragments 2 / 3 load stage s0 + 1 in the first stage)
  int kc = k0, kcs = seg0;  // first row and batch of the stage being multiplied
  // split fragment f (of the stage starting at row kstage of batch kseg) and reload its
  // registers.  The ones column (FILL) loads as zeros (past the record limit), so its
  // lane's split is zero and its ones -- on the batch's rows, none past them -- are set
  // in the high parts: bf16 1.0 per valid row (on the fp32 values before the split: 8
  // more registers).  A clique's panels ascend and the ones column is in the factor's
  // last panel: only its last slot can hold it.
  auto take = [&](int f, int kstage, int kseg, const X3Cursor& c) {
    X3Frag fr = x3_split8(x[f]);
    if (FILL && (DIAG || f == NP - 1)) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const int nv = onesl[f] ? (int)seg_rows(J, kseg) - kstage - lr : 0;  // the lane's valid rows
      u32x4 h = __builtin_bit_cast(u32x4, fr.p[0]);
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] |= (nv > 2 * i ? 0x3f80u : 0u) | (nv > 2 * i + 1 ? 0x3f800000u : 0u);
      fr.p[0] = __builtin_bit_cast(bf16x8, h);
    }
    ld8(f, c, x[f]);
    return fr;
  };
  X3Frag pa = take(0, k0, seg0, c2);
  X3Frag pb = take(1, k0, seg0, c2);
  // the prologue's loads complete here (once per task): the loop header then starts
  // from a precise wait state, and the compiler keeps the counted vmcnt at the top of
  // each stage (with the prologue's loads still in flight it merged them into a
  // vmcnt(0) there, exposing a whole stage of load latency)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // (6 / 11 VALU slots per MFMA measured equal within the box's +-4 us, profiles/r04v/)
  constexpr int NV = FILL ? 52 / 6 + 1 : 44 / 6 + 1;
  // one stage: (F0, F1) of this stage in, (F0', F1') of the next stage out
  auto stage = [&](const X3Frag& F0, const X3Frag& F1, X3Frag& F0n, X3Frag& F1n) {
    const int kn = c2.k, kns = c2.seg;  // first row / batch of the next stage (in x0 / x1 now)
    // the cursors: x2 / x3 reload the next stage, x0 / x1 the one after
    c1 = c2;
    advance(c2);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DIAG) {
      const X3Frag F2 = take(2, kc, kcs, c1);
      x3_six(acc[0], F0, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      const X3Frag F3 = take(3, kc, kcs, c1);
      x3_six(acc[1], F1, F1);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      F0n = take(0, kn, kns, c2);
      x3_six(acc[2], F2, F2);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      F1n = take(1, kn, kns, c2);
      x3_six(acc[3], F3, F3);
      x3_pattern<NV>();
    } else if constexpr (KIND == X3_KS3D3) {
      // (0,0) | split F3    (3,0) | split F2    (1,1) | split F0'
      // (3,1)               (2,2) | split F1'   (3,2)
      // (a K4's six segments and four splits; F0 and F1 end before F0' and F1' are split)
      const X3Frag F3 = take(3, kc, kcs, c1);
      x3_six(acc[3], F0, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      const X3Frag F2 = take(2, kc, kcs, c1);
      x3_six(acc[0], F3, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      F0n = take(0, kn, kns, c2);
      x3_six(acc[4], F1, F1);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[1], F3, F1);
      x3_pattern<0>();
      __builtin_amdgcn_sched_barrier(0);
      F1n = take(1, kn, kns, c2);
      x3_six(acc[5], F2, F2);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[2], F3, F2);
      x3_pattern<0>();
    } else if constexpr (KIND == X3_KP1D2) {
      // (1,0) | split F0'   (0,0) | split F1'   (1,1)
      F0n = take(0, kn, kns, c2);
      x3_six(acc[0], F1, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      F1n = take(1, kn, kns, c2);
      x3_six(acc[1], F0, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[2], F1, F1);
      x3_pattern<0>();
    } else if constexpr (NP == 4) {
      const X3Frag F2 = take(2, kc, kcs, c1);
      x3_six(acc[0], F1, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      const X3Frag F3 = take(3, kc, kcs, c1);
      x3_six(acc[1], F2, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[3], F3, F0);
      x3_pattern<0>();
      __builtin_amdgcn_sched_barrier(0);
      F0n = take(0, kn, kns, c2);
      x3_six(acc[2], F2, F1);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[4], F3, F1);
      x3_pattern<0>();
      __builtin_amdgcn_sched_barrier(0);
      F1n = take(1, kn, kns, c2);
      x3_six(acc[5], F3, F2);
      x3_pattern<NV>();
    } else if constexpr (NP == 3) {
      const X3Frag F2 = take(2, kc, kcs, c1);
      x3_six(acc[0], F1, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      F0n = take(0, kn, kns, c2);
      x3_six(acc[1], F2, F0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      F1n = take(1, kn, kns, c2);
      x3_six(acc[2], F2, F1);
      x3_pattern<NV>();
    } else {  // a single block (1, 0)
      F0n = take(0, kn, kns, c2);
      F1n = take(1, kn, kns, c2);
      x3_six(acc[0], F1, F0);
      x3_pattern<2 * NV>();
    }
    kc = kn;
    kcs = kns;
  };
  // the ragged last batch: sums so far scaled by 1 / rw where the task crosses into it,
  // everything by rw at the end when it reaches it (FactorJobDev::rstage)
  const int64_t rst = J.rstage;
  const int bst = (rst > s0 && rst < s1) ? (int)(rst - s0) : -1;
  for (int st = 0; st < ns; ++st) {
    if (st == bst) scale_acc(acc, J.rinv);
    X3Frag qa, qb;
    stage(pa, pb, qa, qb);
    pa = qa;
    pb = qb;
  }
  if (rst >= 0 && s1 > rst) scale_acc(acc, J.rw);
}

// One unit of kind KIND: its accumulators, the stage loop and the two waves' hand-off.
// The unit's blocks, in accumulator order: block b is (row panel pr, column panel pc),
// sub-block (pr & 1, pc & 1) of 64 x 64 tile (pr >> 1, pc >> 1) of the job's slabs.
// Wave 0 stores the first half of them and wave 1 the rest: each hands the other's
// partials through LDS slot b ([16 values][64 lanes]), then adds the other wave's to
// its own.  Both sums are w0 + w1 (IEEE addition commutes): deterministic.
// (One function per kind, accumulators and all: with one accumulator set shared by the
// kinds' loops the kernel compiled to 251 VGPRs, each kind alone to 187-205.)
template <int KIND>
__device__ __forceinline__ void x3_unit(const FactorJobDev& J, const float* const* segs, const int (&pn)[4],
                                        int np, int split, float* lds) {
  constexpr bool DIAG = KIND == X3_KDIAG;
  constexpr int NB = x3_kind_blocks(KIND);
  const int64_t s0 = (int64_t)split * J.chunk;
  const int64_t s1 = min(J.nst, s0 + J.chunk);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  floatx16 acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[b][v] = 0.f;
  if (s1 > s0) {
    // FILL: one of the unit's fragments holds the ones column (the last panel of an A
    // factor with a bias)
    const int op = J.x.ones >> 5;
    const bool fill = J.x.ones >= 0 && (pn[0] == op || pn[1] == op || pn[2] == op || pn[3] == op);
    if (fill) x3_loop<KIND, true>(J, segs, pn, s0, s1, acc);
    else x3_loop<KIND, false>(J, segs, pn, s0, s1, acc);
  }
  const int nblk = DIAG ? np : NB;  // (a diagonal unit of fewer than four panels)
  constexpr int HALF = (NB + 1) / 2;
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const bool mine = (b < HALF) == (wave == 0);
    if (b < nblk && !mine)
#pragma unroll
      for (int v = 0; v < 16; ++v) lds[(b * 16 + v) * 64 + lane] = acc[b][v];
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const bool mine = (b < HALF) == (wave == 0);
    if (b >= nblk || !mine) continue;
    const X3Block blk = x3_kind_block(KIND, b);  // (b: unrolled, a constant)
    const int pr = pn[blk.i], pc = pn[blk.j];
    const int ti = pr >> 1, tj = pc >> 1;
    float* out = J.slab + ((size_t)(ti * (ti + 1) / 2 + tj) * J.sstride + split) * TILE * TILE +
                 (pr & 1) * 32 * TILE + (pc & 1) * 32;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[b][v] += lds[(b * 16 + v) * 64 + lane];
    put_partial(J, acc[b], [&](int v) { return &out[acc_row(v, lane) * TILE + (lane & 31)]; });
  }
}

template <int GBK>
__device__ __forceinline__ void factor_task_x3(const FactorJobDev& J, const float* const* segs,
                                               const X3Units& U, int unit, int split, float* lds) {
  static_assert(GBK == 16 * X3_NW, "one 16-row half stage per wave");
  const uint32_t u = U.u[J.x3tab + unit];
  const int np = x3_unit_np(u), mix = x3_unit_mix(u);
  const int pn[4] = {x3_unit_panel(u, 0), x3_unit_panel(u, 1), x3_unit_panel(u, 2), x3_unit_panel(u, 3)};
  switch (mix == X3_MIX_S3D3 ? X3_KS3D3 : mix == X3_MIX_P1D2 ? X3_KP1D2 : (u & X3_DIAG) ? X3_KDIAG : np) {
    case 4: x3_unit<4>(J, segs, pn, np, split, lds); break;
    case 3: x3_unit<3>(J, segs, pn, np, split, lds); break;
    case 2: x3_unit<2>(J, segs, pn, np, split, lds); break;
    case X3_KDIAG: x3_unit<X3_KDIAG>(J, segs, pn, np, split, lds); break;
    case X3_KS3D3: x3_unit<X3_KS3D3>(J, segs, pn, np, split, lds); break;
    case X3_KP1D2: x3_unit<X3_KP1D2>(J, segs, pn, np, split, lds); break;
    default: break;  // (not reached)
  }
}

// Every job of the launch is LDS-DMA-eligible or narrow (n <= 32: direct loads).
// 2 waves per SIMD: 4 workgroups per CU leave a 32-tile inversion workgroup (107
// registers, 29 KB) room to run beside the pass
__global__ __launch_bounds__(X3_THREADS, 2) void kfac_factor_tiles_x3(FactorArgs args, X3Units units) {
  // (LDS only for the epilogue's hand-off: a K4's six blocks, 24 KB)
  __shared__ __attribute__((aligned(16))) float lds[X3_NACC * 16 * 64];
  // (no start stagger here: the fp32 kernel's +2.5 % measured neutral on this one, MLP
  // line 1.951-1.954e8 without vs 1.951-1.957e8 with, 3 alternating runs, profiles/r06b/)
  int j = 0, unit, split;
  if (args.split_major == 2) {
    // every job at the same K-splits: split-major across the launch (factor_common.h;
    // task_end counts units here)
    x3_task_decode(args.task_end, args.njobs, args.job[0].splits, gridDim.x, blockIdx.x, j, unit, split);
  } else {
    const int task = xcd_task(blockIdx.x, gridDim.x);
    while (j + 1 < args.njobs && task >= args.task_end[j]) ++j;
    const int local = task - args.job[j].task_begin;
    const int nu = args.job[j].x3units, ns = args.job[j].splits;
    split = args.split_major ? local / nu : local % ns;
    unit = args.split_major ? local - split * nu : local / ns;
  }
  const FactorJobDev& J = args.job[j];
  if (J.n <= 32)
    factor_task_narrow_direct<X3_NW>(J, args.segs, split, lds);
  else
    factor_task_x3<BK>(J, args.segs, units, unit, split, lds);
}

// ------------------------------------------------------------------- host side
namespace {

uint32_t x3_pack(const int* p, int np, bool diag, int mix = 0) {
  uint32_t u = (uint32_t)np << 24 | (diag ? X3_DIAG : 0u) | (uint32_t)mix << 29;
  for (int s = 0; s < 4; ++s) u |= (uint32_t)p[std::min(s, np - 1)] << (6 * s);
  return u;
}

// The table of P panels.  P = 25: the 25 translates of two base blocks of the affine plane
// coordinates (x, y) of Z5 x Z5, panel 5 x + y -- {(0,0), (0,1), (1,0), (2,2)} and twice
// it; their 24 differences are the 24 non-zero vectors, each once, so every panel pair
// lies in exactly one of the 50 blocks (a Steiner system S(2, 4, 25)).  Any other P: the
// first K4 in lexicographic order whose six pairs are all free, until none is left, then
// K3s the same way.  The pairs still free then -- one unit each as K2s -- are taken with
// diagonal blocks where that saves units: three of them under one higher panel h, to
// panels a < b < c whose diagonal blocks are free, are one S3D3 (a, b, c, h); a pair whose
// two diagonal blocks are free is a P1D2; the rest are K2s, and the diagonal blocks still
// free go four to a diagonal unit.  A pair or a diagonal block is never taken twice, and
// the K2 and diagonal passes take every one still free, so the partition is exact
// whatever the packing's quality.  (The K3s come before the mixed units: an S3D3 then
// replaces three K2s and three quarters of a diagonal unit, a P1D2 one K2 and half of
// one, so no P has more units than with cliques and diagonal units alone.)
std::vector<uint32_t> x3_build_table(int P) {
  std::vector<uint32_t> k4, s3, k3, p1, k2, dg;
  std::vector<char> used((size_t)P * P, 0), dused(P, 0);
  auto is_free = [&](int a, int b) { return !used[(size_t)a * P + b]; };
  auto mark = [&](int a, int b) { used[(size_t)a * P + b] = used[(size_t)b * P + a] = 1; };
  if (P == 25) {
    const int base[4][2] = {{0, 0}, {0, 1}, {1, 0}, {2, 2}};
    for (int m = 1; m <= 2; ++m)
      for (int sx = 0; sx < 5; ++sx)
        for (int sy = 0; sy < 5; ++sy) {
          int p[4];
          for (int i = 0; i < 4; ++i) p[i] = 5 * ((m * base[i][0] + sx) % 5) + (m * base[i][1] + sy) % 5;
          std::sort(p, p + 4);
          for (int i = 0; i < 4; ++i)
            for (int j = 0; j < i; ++j) mark(p[i], p[j]);
          k4.push_back(x3_pack(p, 4, false));
        }
  }
  for (int a = 0; a < P; ++a)
    for (int b = a + 1; b < P; ++b) {
      if (!is_free(a, b)) continue;
      for (int c = b + 1; c < P && is_free(a, b); ++c) {
        if (!is_free(a, c) || !is_free(b, c)) continue;
        for (int d = c + 1; d < P; ++d)
          if (is_free(a, d) && is_free(b, d) && is_free(c, d)) {
            const int p[4] = {a, b, c, d};
            for (int i = 0; i < 4; ++i)
              for (int j = 0; j < i; ++j) mark(p[i], p[j]);
            k4.push_back(x3_pack(p, 4, false));
            break;
          }
      }
    }
  for (int a = 0; a < P; ++a)
    for (int b = a + 1; b < P; ++b)
      for (int c = b + 1; c < P && is_free(a, b); ++c)
        if (is_free(a, c) && is_free(b, c)) {
          const int p[3] = {a, b, c};
          mark(a, b), mark(a, c), mark(b, c);
          k3.push_back(x3_pack(p, 3, false));
        }
  for (int h = 0; h < P; ++h) {  // the stars of the hub h
    int p[4], np = 0;
    for (int a = 0; a < h; ++a) {
      if (!is_free(a, h) || dused[a]) continue;
      p[np++] = a;
      if (np < 3) continue;
      p[3] = h;
      for (int i = 0; i < 3; ++i) mark(p[i], h), dused[p[i]] = 1;
      s3.push_back(x3_pack(p, 4, false, X3_MIX_S3D3));
      np = 0;
    }
  }
  for (int a = 0; a < P; ++a)
    for (int b = a + 1; b < P; ++b) {
      if (!is_free(a, b)) continue;
      const int p[2] = {a, b};
      mark(a, b);
      if (!dused[a] && !dused[b]) {
        dused[a] = dused[b] = 1;
        p1.push_back(x3_pack(p, 2, false, X3_MIX_P1D2));
      } else {
        k2.push_back(x3_pack(p, 2, false));
      }
    }
  {
    int p[4], np = 0;
    for (int a = 0; a < P; ++a) {
      if (!dused[a]) p[np++] = a;
      if (np == 4 || (np > 0 && a == P - 1)) {
        dg.push_back(x3_pack(p, np, true));
        np = 0;
      }
    }
  }
  std::vector<uint32_t> t(k4);
  t.insert(t.end(), s3.begin(), s3.end());
  t.insert(t.end(), dg.begin(), dg.end());
  t.insert(t.end(), k3.begin(), k3.end());
  t.insert(t.end(), p1.begin(), p1.end());
  t.insert(t.end(), k2.begin(), k2.end());
  return t;
}

}  // namespace

int x3_unit_table(int P, const uint32_t** table) {
  static std::mutex mu;
  static std::vector<uint32_t> tables[X3_PMAX + 1];
  if (P < 2 || P > X3_PMAX) return 0;
  std::lock_guard<std::mutex> lock(mu);
  if (tables[P].empty()) tables[P] = x3_build_table(P);
  if (table) *table = tables[P].data();
  return (int)tables[P].size();
}

int x3_units(int n) { return n <= 32 ? 1 : x3_unit_table(x3_panels(n), nullptr); }

int x3_table_entries(const int* n, int njobs) {
  bool seen[X3_PMAX + 1] = {};
  int total = 0;
  for (int i = 0; i < njobs; ++i) {
    const int P = x3_panels(n[i]);
    if (n[i] <= 32 || P > X3_PMAX || seen[P]) continue;
    seen[P] = true;
    total += x3_unit_table(P, nullptr);
  }
  return total;
}

// The launch's unit tables go with the kernel arguments: one copy per distinct P, each
// job pointed at its own (x3tab; the router keeps a group within X3_UCAP entries).
int launch_tiles_x3(const FactorArgs& args, int tasks, hipStream_t stream) {
  FactorArgs a = args;
  X3Units U;
  int off[X3_PMAX + 1], total = 0;
  std::fill(off, off + X3_PMAX + 1, -1);
  for (int i = 0; i < a.njobs; ++i) {
    FactorJobDev& d = a.job[i];
    d.x3tab = 0;
    if (d.n <= 32) continue;
    const int P = x3_panels(d.n);
    const uint32_t* t = nullptr;
    const int nu = x3_unit_table(P, &t);
    if (nu == 0 || nu != d.x3units) return KFAC_ELAUNCH;
    if (off[P] < 0) {
      if (total + nu > X3_UCAP) return KFAC_ELAUNCH;
      std::copy(t, t + nu, U.u + total);
      off[P] = total;
      total += nu;
    }
    d.x3tab = off[P];
  }
  std::fill(U.u + total, U.u + X3_UCAP, 0u);
  hipLaunchKernelGGL(kfac_factor_tiles_x3, dim3(tasks), dim3(X3_THREADS), 0, stream, a, U);
  return KFAC_OK;
}

}  // namespace kfac

// The unit table of P panels, unpacked for inspection (include/kfac_hip.h)
extern "C" int kfac_x3_unit_table(int P, int32_t* out, int cap) {
  const uint32_t* t = nullptr;
  const int nu = kfac::x3_unit_table(P, &t);
  for (int i = 0; i < nu && i < cap && out; ++i) {
    const int np = kfac::x3_unit_np(t[i]);
    const bool diag = (t[i] & kfac::X3_DIAG) != 0;
    const int mix = kfac::x3_unit_mix(t[i]);
    for (int s = 0; s < 4; ++s) out[6 * i + s] = s < np ? kfac::x3_unit_panel(t[i], s) : -1;
    out[6 * i + 4] = mix == kfac::X3_MIX_S3D3 ? 0b110100 : mix == kfac::X3_MIX_P1D2 ? 0b000001
                     : diag ? 0 : (np == 4 ? 63 : np == 3 ? 0b001011 : 0b000001);
    out[6 * i + 5] = mix == kfac::X3_MIX_S3D3 ? 0b0111 : mix == kfac::X3_MIX_P1D2 ? 0b0011
                     : diag ? (1 << np) - 1 : 0;
  }
  return nu;
}

// Workgroup `block`'s task in the launch-wide split-major order (include/kfac_hip.h)
extern "C" int kfac_x3_task_decode(const int32_t* units, int njobs, int splits, int blocks, int block,
                                   int32_t* xcd_job_unit_split) {
  if (!units || !xcd_job_unit_split || njobs < 1 || njobs > kfac::MAXJ || splits < 1) return KFAC_EINVAL;
  int64_t U = 0;
  int unit_end[kfac::MAXJ];
  for (int i = 0; i < njobs; ++i) {
    if (units[i] < 1 || units[i] > kfac::X3_UCAP) return KFAC_EINVAL;
    U += units[i];
    unit_end[i] = (int)U;
  }
  if (U * splits != blocks || block < 0 || block >= blocks) return KFAC_EINVAL;
  int job, unit, split;
  kfac::x3_task_decode(unit_end, njobs, splits, blocks, block, job, unit, split);
  xcd_job_unit_split[0] = block & 7;
  xcd_job_unit_split[1] = job;
  xcd_job_unit_split[2] = unit;
  xcd_job_unit_split[3] = split;
  return KFAC_OK;
}
