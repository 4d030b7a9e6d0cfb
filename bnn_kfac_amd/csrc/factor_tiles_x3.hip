#include <type_traits>

#include "bf16x3.h"
#include "factor_common.h"

namespace kfac {

// ------------------------------- fp32 operands, bf16x3 products split in registers
// kfac_factor_tiles_x3: TWO waves per 64 x 64 tile, each computing the WHOLE tile over
// its own 16-row half of every 32-row stage.  A lane loads its MFMA fragment -- 8
// consecutive k of one column -- straight from global memory into registers (no LDS),
// splits it (split3: the exact three-part split of the bf16x3 kernels above) and the
// wave runs six v_mfma_f32_32x32x16_bf16 per 32 x 32 block: 24 MFMAs of 32 cycles per
// wave and 16-row half, against the fp32 kernel's 4 waves x 8 fp32 MFMAs of 64 cycles
// for the same work, with no split pass and no padded images (the n <= 1024 factors,
// where kfac_split3's HBM round trip costs as much as the products).  The two waves'
// partial tiles are summed through LDS in a fixed order at the end.
// Measured on the MNIST MLP group (profiles/r03_x3/ab/probe_summary.txt): direct loads
// beat LDS-DMA rings (shared, one barrier per stage, or one per wave without a
// barrier: 179 vs 196-204 us per 32,768-row launch), the compiled split beats a
// hand-ordered asm one, and 128 x 128 macro tiles with the split made once per macro
// tile into the syrk3 LDS image (x3m) lost (224 us).  The kernel is issue-bound: two
// waves per SIMD keep its issue port ~90 % busy with 7.3 split VALU per MFMA.
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

// The stage loop (round 4): software-pipelined segments in ONE straight-line block.
// The fragments of the stage's first block -- A0 (and B0) -- are split during the
// previous stage; every segment is the six MFMAs of one block interleaved
// (sched_group_barrier) with the split of a fragment a later block needs, and that
// fragment's registers are reloaded as soon as its split has read them:
//   full tile (mask 15):  (0,0) | split A1    (1,0) | split B1    (0,1) | split A0'
//                         (1,1) | split B0'
// so each load goes out one whole stage before its split (x1, x3 hold the next stage,
// x0, x2 the one after), at most five fragments are live and no register set is copied
// (2 waves per SIMD at <= 200 VGPRs leave an inversion wave room beside them).  Round 3's
// loop split all four fragments at the top of the stage, copied a 32-register prefetch
// set into the working set every stage, branched per stage (last stage, batch change,
// fill columns with 64-bit compares), and the compiler sank every load to the end of
// the body and waited vmcnt(0) at the loop head: ~100 extra VALU and the whole L2
// latency per stage.  Now every load is unconditional: past the task's range the
// cursor stops (the last stage reloads itself), a batch change is a scalar select (the
// next batch's base fetched a stage ahead), columns past the operand load from past
// the buffer's record limit (0), and the ones column (FILL: only the tasks whose
// fragments hold it) is a select of 1 / 0 by row validity.
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

// X3_PAIR: a factor whose last tile row is thin (n - 64 (T-1) <= 32: one block row,
// the MNIST MLP's 785 and 129) pairs diagonal tile (i, i) with edge tile (T-1, i) in ONE
// task: fragments A0, A1 (panel i) and C0 (panel T-1, block 0), five blocks
//   D00 = A0 A0, D10 = A1 A0, D11 = A1 A1 (tile (i, i)), E00 = C0 A0, E01 = C0 A1
// -- 30 MFMAs on 3 fragments per 16 rows, where the diagonal task alone did 18 on 2
// and the edge task 12 on 3 (both ran ahead of the full tiles, widening each XCD's
// L2 working set), and T-1 fewer tasks per K-split.  acc[0][0] D00, acc[1][0] D10,
// acc[1][1] D11, acc[0][1] E00, acc4 E01; called with ti = i, tj = T-1.
constexpr int X3_PAIR = 16;

template <int MASK, bool FILL>
__device__ __forceinline__ void x3_loop(const FactorJobDev& J, const float* const* segs, int ti, int tj,
                                        int64_t s0, int64_t s1, floatx16 (&acc)[2][2], floatx16& acc4) {
  constexpr bool PAIR = MASK == X3_PAIR;
  constexpr bool A00 = MASK & 1, A01 = MASK & 2, A10 = MASK & 4, A11 = MASK & 8;
  constexpr bool ROW1 = A10 || A11 || PAIR, COL1 = A01 || A11;
  // masks 13 and 1 occur on diagonal tiles only (an off-diagonal tile with block
  // (1, 1), or with any block, has (0, 1)): B fragments = A fragments
  constexpr bool SAME = MASK == 13 || MASK == 1;
  static_assert(A00 || PAIR, "block (0, 0) always has work");
  // fragments: 0 A block 0, 1 A block 1, 2 B block 0, 3 B block 1 (PAIR: 2 = C0)
  constexpr bool USE[4] = {true, ROW1, !SAME, !SAME && COL1};
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
    const int c = (f < 2 ? ti : tj) * TILE + (f & 1) * 32 + (lane & 31);
    voff[f] = c < J.x.cols ? lr * ld4 + c * 4 : rec;  // past the operand: the zero tail
    onesl[f] = c == J.x.ones;
  }
  const int ns = (int)(s1 - s0);
  const int lastseg = J.nseg - 1;
  // stage cursors: c1 = the next stage to load for fragments 1 / 3, c2 = the one after
  // (fragments 0 / 2); nb = the base of the batch after c2's
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
  for (int f = 0; f < 4; ++f)
    if (USE[f]) ld8(f, c2, x[f]);
  advance(c2);
  X3Cursor c1 = c2;  // (fragments 1 / 3 load stage s0 + 1 in the first stage)
  int kc = k0, kcs = seg0;  // first row and batch of the stage being multiplied
  auto fix = [&](int f, int kstage, int kseg) {  // the ones column: 1 on the batch's rows, 0 past them
    if constexpr (FILL) {
      const int nvalid = (int)seg_rows(J, kseg) - kstage;
#pragma unroll
      for (int r = 0; r < 8; ++r) x[f][r] = onesl[f] ? (lr + r < nvalid ? 1.f : 0.f) : x[f][r];
    }
  };
  // split fragment f (of the stage starting at row kstage of batch kseg) and reload its
  // registers
  auto take = [&](int f, int kstage, int kseg, const X3Cursor& c) {
    fix(f, kstage, kseg);
    const X3Frag fr = x3_split8(x[f]);
    ld8(f, c, x[f]);
    return fr;
  };
  X3Frag pa = take(0, k0, seg0, c2);
  X3Frag pb = SAME ? pa : take(2, k0, seg0, c2);
  // the prologue's loads complete here (once per task): the loop header then starts
  // from a precise wait state, and the compiler keeps the counted vmcnt at the top of
  // each stage (with the prologue's loads still in flight it merged them into a
  // vmcnt(0) there, exposing a whole stage of load latency)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // (6 / 11 VALU slots per MFMA measured equal within the box's +-4 us, profiles/r04v/)
  constexpr int NV = FILL ? 52 / 6 + 1 : 44 / 6 + 1;
  // one stage: P = (A0, B0) of this stage in, (A0', B0') of the next stage out
  auto stage = [&](const X3Frag& A0, const X3Frag& B0, X3Frag& A0n, X3Frag& B0n) {
    const int kn = c2.k, kns = c2.seg;  // first row / batch of the next stage (in x0 / x2 now)
    // the cursors: x1 / x3 reload the next stage, x0 / x2 the one after
    c1 = c2;
    advance(c2);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (PAIR) {  // B0 = C0
      const X3Frag A1 = take(1, kc, kcs, c1);
      x3_six(acc[0][0], A0, A0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      A0n = take(0, kn, kns, c2);
      x3_six(acc[0][1], B0, A0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      B0n = take(2, kn, kns, c2);
      x3_six(acc[1][0], A1, A0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[1][1], A1, A1);
      x3_pattern<0>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc4, B0, A1);
      x3_pattern<0>();
    } else if constexpr (MASK == 15) {
      const X3Frag A1 = take(1, kc, kcs, c1);
      x3_six(acc[0][0], A0, B0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      const X3Frag B1 = take(3, kc, kcs, c1);
      x3_six(acc[1][0], A1, B0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      A0n = take(0, kn, kns, c2);
      x3_six(acc[0][1], A0, B1);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      B0n = take(2, kn, kns, c2);
      x3_six(acc[1][1], A1, B1);
      x3_pattern<NV>();
    } else if constexpr (MASK == 13) {  // diagonal: (0,0) (1,0) (1,1), B = A
      const X3Frag A1 = take(1, kc, kcs, c1);
      x3_six(acc[0][0], A0, A0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[1][0], A1, A0);
      A0n = take(0, kn, kns, c2);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      x3_six(acc[1][1], A1, A1);
      x3_pattern<0>();
      B0n = A0n;
    } else if constexpr (MASK == 5) {  // (0,0) (1,0)
      const X3Frag A1 = take(1, kc, kcs, c1);
      x3_six(acc[0][0], A0, B0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      A0n = take(0, kn, kns, c2);
      B0n = take(2, kn, kns, c2);
      x3_six(acc[1][0], A1, B0);
      x3_pattern<2 * NV>();
    } else if constexpr (MASK == 3) {  // (0,0) (0,1): the last tile row of a factor
      const X3Frag B1 = take(3, kc, kcs, c1);
      x3_six(acc[0][0], A0, B0);
      x3_pattern<NV>();
      __builtin_amdgcn_sched_barrier(0);
      A0n = take(0, kn, kns, c2);
      B0n = take(2, kn, kns, c2);
      x3_six(acc[0][1], A0, B1);
      x3_pattern<2 * NV>();
    } else {  // 1: the last diagonal tile, (0,0) only, B = A
      A0n = take(0, kn, kns, c2);
      x3_six(acc[0][0], A0, A0);
      x3_pattern<NV>();
      B0n = A0n;
    }
    kc = kn;
    kcs = kns;
  };
  // the ragged last batch: sums so far scaled by 1 / rw where the task crosses into it,
  // everything by rw at the end when it reaches it (FactorJobDev::rstage)
  const int64_t rst = J.rstage;
  const int bst = (rst > s0 && rst < s1) ? (int)(rst - s0) : -1;
  for (int st = 0; st < ns; ++st) {
    if (st == bst) {
      scale_acc(acc[0], J.rinv);
      scale_acc(acc[1], J.rinv);
      if constexpr (PAIR) {
        floatx16 a4[1] = {acc4};
        scale_acc(a4, J.rinv);
        acc4 = a4[0];
      }
    }
    X3Frag qa, qb;
    stage(pa, pb, qa, qb);
    pa = qa;
    pb = qb;
  }
  if (rst >= 0 && s1 > rst) {
    scale_acc(acc[0], J.rw);
    scale_acc(acc[1], J.rw);
    if constexpr (PAIR) {
      floatx16 a4[1] = {acc4};
      scale_acc(a4, J.rw);
      acc4 = a4[0];
    }
  }
}

template <int GBK, int NSLOT>
__device__ __forceinline__ void factor_task_x3(const FactorJobDev& J, const float* const* segs, int local,
                                               float* lds, int split_major) {
  static_assert(GBK == 16 * X3_NW, "one 16-row half stage per wave");
  const int T = J.t;
  const bool thin = J.x3pair != 0;
  const int units = x3_units_of(T, thin);
  const int sf = J.splits - J.xsplits;  // the full K-splits (every unit)
  int split, unit;
  if (local >= units * sf) {  // the pair units' extra K-splits (x3_xsplits)
    const int e = local - units * sf;
    split = sf + e / (T - 1);
    unit = e - (split - sf) * (T - 1);
  } else {
    split = split_major ? local / units : local % sf;
    unit = split_major ? local - split * units : local / sf;
  }
  int ti, tj;
  bool pair = false;
  if (!thin) {
    tri_decode(unit, ti, tj);
  } else if (unit < T - 1) {  // pairs first: diagonal (i, i) with edge (T-1, i)
    pair = true;
    ti = unit;
    tj = T - 1;
  } else if (unit < T - 1 + (T - 1) * (T - 2) / 2) {  // strictly lower tiles of rows < T-1
    tri_decode(unit - (T - 1), ti, tj);
    ++ti;  // (row i of the strict lower triangle has i tiles: tri index of (i-1, j))
  } else {  // the corner (T-1, T-1)
    ti = tj = T - 1;
  }
  const int tile = ti * (ti + 1) / 2 + (pair ? ti : tj);  // (a pair's: its diagonal tile)
  // a pair unit's K-chunk: nst over all `splits` slabs; the others' over the full splits
  const int64_t chunk = pair && J.xsplits ? (J.nst + J.splits - 1) / J.splits : J.chunk;
  const int64_t s0 = (int64_t)split * chunk;
  const int64_t s1 = min(J.nst, s0 + chunk);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const bool same = ti == tj;
  bool act[2][2];
  int mask = 0;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      act[bi][bj] = !(same && bi < bj) && ti * TILE + bi * 32 < J.n && tj * TILE + bj * 32 < J.n;
      mask |= act[bi][bj] << (2 * bi + bj);
    }
  if (pair) mask = X3_PAIR;
  floatx16 acc[2][2], acc4;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[bi][bj][v] = 0.f;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc4[v] = 0.f;
  if (s1 > s0) {
    // FILL: one of the task's fragments holds the ones column (the last tile row /
    // column of an A factor with a bias)
    const bool fill = J.x.ones >= 0 && ((J.x.ones >> 6) == ti || (J.x.ones >> 6) == tj);
#define X3_CASE(M)                                                   \
  case M:                                                            \
    if (fill) x3_loop<M, true>(J, segs, ti, tj, s0, s1, acc, acc4);  \
    else x3_loop<M, false>(J, segs, ti, tj, s0, s1, acc, acc4);      \
    break;
    switch (mask) {  // (block (0, 0) always has work)
      X3_CASE(X3_PAIR)
      X3_CASE(15)
      X3_CASE(13)  // diagonal
      X3_CASE(5)
      X3_CASE(3)
      X3_CASE(1)
      default: break;  // (not reached)
    }
#undef X3_CASE
  }
  if (pair) {
    // wave 0 keeps D00, E00, E01 and wave 1 D10, D11; each hands the other's through
    // LDS slots [D00, D10, D11, E00, E01][16 values][64 lanes]; sums are w0 + w1
    __syncthreads();
    float* xo = lds;
    auto put = [&](int sl, const floatx16& a) {
#pragma unroll
      for (int v = 0; v < 16; ++v) xo[(sl * 16 + v) * 64 + lane] = a[v];
    };
    auto add = [&](int sl, floatx16& a) {
#pragma unroll
      for (int v = 0; v < 16; ++v) a[v] += xo[(sl * 16 + v) * 64 + lane];
    };
    float* outD = J.slab + ((size_t)tile * J.sstride + split) * TILE * TILE;
    float* outE = J.slab + ((size_t)((T - 1) * T / 2 + ti) * J.sstride + split) * TILE * TILE;
    auto store = [&](float* o, int bi, int bj, const floatx16& a) {
      put_partial(J, a, [&](int v) { return &o[(bi * 32 + acc_row(v, lane)) * TILE + bj * 32 + (lane & 31)]; });
    };
    if (wave == 0) {
      put(1, acc[1][0]);
      put(2, acc[1][1]);
    } else {
      put(0, acc[0][0]);
      put(3, acc[0][1]);
      put(4, acc4);
    }
    __syncthreads();
    if (wave == 0) {
      add(0, acc[0][0]);
      add(3, acc[0][1]);
      add(4, acc4);
      store(outD, 0, 0, acc[0][0]);
      store(outE, 0, 0, acc[0][1]);
      store(outE, 0, 1, acc4);
    } else {
      add(1, acc[1][0]);
      add(2, acc[1][1]);
      store(outD, 1, 0, acc[1][0]);
      store(outD, 1, 1, acc[1][1]);
    }
    return;
  }
  // wave w stores block row w: it hands the other block row's partials to the other
  // wave through LDS (the ring is free after the barrier), then adds the other
  // wave's.  Both sums are w0 + w1 (IEEE addition commutes): deterministic.
  __syncthreads();
  float* xo = lds;  // [wave][bj][16 values][64 lanes]
  float* out = J.slab + ((size_t)tile * J.sstride + split) * TILE * TILE;
  auto hand = [&](auto bic) {
    constexpr int bi = decltype(bic)::value;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
      if (act[bi][bj])
#pragma unroll
        for (int v = 0; v < 16; ++v) xo[((wave * 2 + bj) * 16 + v) * 64 + lane] = acc[bi][bj][v];
  };
  auto keep = [&](auto bic) {
    constexpr int bi = decltype(bic)::value;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
      if (act[bi][bj]) {
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[bi][bj][v] += xo[(((1 - wave) * 2 + bj) * 16 + v) * 64 + lane];
        put_partial(J, acc[bi][bj],
                    [&](int v) { return &out[(bi * 32 + acc_row(v, lane)) * TILE + bj * 32 + (lane & 31)]; });
        // the slabs of the pair units' extra K-splits hold nothing of this tile: its
        // last full K-split writes them as zero partials
        if (split == sf - 1)
          for (int x = 1; x <= J.xsplits; ++x) {
            floatx16 z;
#pragma unroll
            for (int v = 0; v < 16; ++v) z[v] = 0.f;
            float* o = out + (size_t)x * TILE * TILE;
            put_partial(J, z, [&](int v) { return &o[(bi * 32 + acc_row(v, lane)) * TILE + bj * 32 + (lane & 31)]; });
          }
      }
  };
  if (wave == 0) hand(std::integral_constant<int, 1>{});
  else hand(std::integral_constant<int, 0>{});
  __syncthreads();
  if (wave == 0) keep(std::integral_constant<int, 0>{});
  else keep(std::integral_constant<int, 1>{});
}

// Every job of the launch is LDS-DMA-eligible or narrow (n <= 32: direct loads).
// 2 waves per SIMD (178 VGPRs): 4 workgroups per CU leave a 32-tile inversion
// workgroup (107 registers, 29 KB) room to run beside the pass
__global__ __launch_bounds__(X3_THREADS, 2) void kfac_factor_tiles_x3(FactorArgs args) {
  // (LDS only for the epilogue's hand-off: a block row, 16 KB; a pair's blocks, 20 KB)
  __shared__ __attribute__((aligned(16))) float lds[5 * 16 * 64];
  // (no start stagger here: the fp32 kernel's +2.5 % measured neutral on this one, MLP
  // line 1.951-1.954e8 without vs 1.951-1.957e8 with, 3 alternating runs, profiles/r06b/)
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int j = 0;
  while (j + 1 < args.njobs && task >= args.task_end[j]) ++j;
  const int local = task - args.job[j].task_begin;
  const FactorJobDev& J = args.job[j];
  if (J.n <= 32)
    factor_task_narrow_direct<X3_NW>(J, args.segs, local, lds);
  else
    factor_task_x3<BK, 2>(J, args.segs, local, lds, args.split_major);
}

// ------------------------------------------------------------------- host side
int launch_tiles_x3(const FactorArgs& args, int tasks, hipStream_t stream) {
  hipLaunchKernelGGL(kfac_factor_tiles_x3, dim3(tasks), dim3(X3_THREADS), 0, stream, args);
  return KFAC_OK;
}

}  // namespace kfac
