#include "bf16x3.h"
#include "factor_common.h"

namespace kfac {

// ------------------------------------------------- bf16x3 split SYRK (row-major)
// fp32-accurate products on the bf16 matrix cores.  Every operand element is split
// EXACTLY into three bf16 parts, x = x1 + x2 + x3 (round-to-nearest splits: x1 holds
// the top 8 significant bits, x2 the next 8, x3 the last 8 of fp32's 24), and
//   x_a x_b = x1a x1b + (x1a x2b + x2a x1b) + (x1a x3b + x2a x2b + x3a x1b) + O(2^-24)
// -- six bf16 MFMA products per fp32 product, the dropped terms (x2 x3, x3 x2, x3 x3)
// below fp32's own rounding of the product, accumulated in fp32 by the MFMA.  On
// gfx950 v_mfma_f32_32x32x16_bf16 retires 16x the FLOP/cycle of the fp32 MFMA
// (v_mfma_f32_32x32x2_f32), so six of them are 2.67x the fp32 MFMA rate: the
// roofline of this kernel is 2.5 PF / 6 = 417 TF/s of fp32-equivalent work.
//
// kfac_factor_syrk3: one 128 x 128 macro tile (= 2 x 2 of the 64-tiles whose partial
// slabs the reduce sums) of one factor over one K-chunk per workgroup; the workgroup
// loads each 16-row substep of its panels once, splits it into the LDS image below and
// its 4 waves multiply from there (s3q_task).  Until round 5 a separate kfac_split3
// pass wrote the split images to HBM (6 B per operand element) and the SYRK read them
// back by LDS-DMA.
// LDS image of a substep: [part][column][2 chunks of 8 k] (32 B per column, k
// contiguous), read straight into MFMA operands (lane = column, 8 k per
// ds_read_b128); the chunk of a column is XOR-swizzled (s3_half), so the fragment
// reads and the split's writes are conflict-free and each read is a per-lane base plus
// an immediate.
// (A first version split in 8 producer waves beside 4 consumer waves per workgroup:
// producer-bound at 0.25 of the roofline)
constexpr int MT = 128;                          // macro tile edge
constexpr int S3_PART = 2 * MT * 32;             // bytes of one part of a substep slot (A and B)
constexpr int S3_REG = 3 * S3_PART + 64;         // one substep slot (+64: bank offset)

// byte offset of half-chunk hh (k 8hh .. 8hh+7 of a substep) of column c in a part.
// The half is swapped by bit 2 ^ bit 3 of the column: the fragment reads (ds_read_b128,
// lane groups {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31}) and the split's writes
// (ds_write_b128, 8 consecutive columns) both hit distinct bank quads (bit 3 alone left
// the writes 2-way conflicted: 2.7 conflict cycles per LDS instruction, profiles/r06a_wide/)
__device__ __forceinline__ int s3_half(int c, int hh) { return c * 32 + ((hh ^ (((c >> 2) ^ (c >> 3)) & 1)) << 4); }

// A wave's MFMAs on one 16-row k-substep (the slot at `reg`): blocks (bi, bj) of its
// 64 x 64 quadrant with act[bi][bj], six products per block.  oa / ob: this lane's A / B
// fragment offsets (part 0, block 0); everything else is an immediate.  The 12
// fragments go out first, then the MFMAs.
__device__ __forceinline__ void s3_consume_sub(const char* reg, int oa, int ob, const bool (&act)[2][2],
                                               floatx16 (&acc)[2][2]) {
  auto frag = [&](int off) { return *reinterpret_cast<const bf16x8*>(reg + off); };
  auto six = [&](int bi, int bj, const bf16x8* A, const bf16x8* B) {
    if (!act[bi][bj]) return;
    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2], B[0], acc[bi][bj], 0, 0, 0);
    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], B[1], acc[bi][bj], 0, 0, 0);
    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[2], acc[bi][bj], 0, 0, 0);
    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[1], B[0], acc[bi][bj], 0, 0, 0);
    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[1], acc[bi][bj], 0, 0, 0);
    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[0], B[0], acc[bi][bj], 0, 0, 0);
  };
  bf16x8 a0[3], a1[3], b0[3], b1[3];
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    a0[p] = frag(oa + p * S3_PART);
    b0[p] = frag(ob + p * S3_PART);
    b1[p] = frag(ob + p * S3_PART + 32 * 32);
    a1[p] = frag(oa + p * S3_PART + 32 * 32);
  }
  six(0, 0, a0, b0);
  six(0, 1, a0, b1);
  six(1, 0, a1, b0);
  six(1, 1, a1, b1);
}

// Macro tile of a unit index, in blocks of 4 tile rows x 8 tile columns of the lower
// triangle: the ~32 tasks an XCD runs at once (xcd_task hands it a contiguous range)
// then read 4 A panels and 8 B panels, not 1 and 32, so a stage's rows are fetched
// into its L2 once per panel block instead of once per task (wide factors: 4096
// columns = 32 panels of 128 each far larger than the 4 MB L2).
__device__ __forceinline__ void s3_decode(int unit, int T3, int& I, int& J) {
  int base = 0;
  I = J = 0;
  for (int i0 = 0; i0 < T3; i0 += 4) {
    const int i1 = min(T3, i0 + 4);
    for (int j0 = 0; j0 < i1; j0 += 8) {
      int cnt = 0;
      for (int i = i0; i < i1; ++i) cnt += max(0, min(j0 + 8, i + 1) - j0);
      if (unit < base + cnt) {
        int r = unit - base;
        for (int i = i0; i < i1; ++i) {
          const int w = max(0, min(j0 + 8, i + 1) - j0);
          if (r < w) {
            I = i;
            J = j0 + r;
            return;
          }
          r -= w;
        }
      }
      base += cnt;
    }
  }
}

// ------------------------------------- bf16x3 SYRK, split once per workgroup
// (round 5; replaces the separate split pass).  One 128 x 128 macro
// tile of one factor over one K-chunk per workgroup of 4 waves, 2 workgroups per CU.
// Per 16-row substep, thread t loads column t of the [A panel | B panel] (256 columns)
// -- 16 rows, two 8-row halves, buffer loads whose record limit zero-fills rows past
// the batch and columns past the operand -- splits it into its three bf16 parts and
// writes them as the substep's LDS image (the layout above: [part][column][2 halves],
// half swizzled by bit 3 of the column).  Two slots: while the waves' MFMAs consume
// substep h from one, the split of substep h + 1 goes into the other, interleaved with
// those MFMAs (sched_group_barrier), and the loads of substep h + 2 are in flight.
// One barrier per substep.  Each wave computes its 64 x 64 quadrant (w >> 1, w & 1)
// as 2 x 2 blocks, six products per block: 24 MFMAs per substep against 2 columns x
// 16 values split per thread (3.7 VALU per MFMA; tools/microbench/cutq_mb.hip: 0.448
// of 417 TF/s on a 4096-column operand).
constexpr int S3D_LDS = 2 * S3_REG;

template <bool FILL>
__device__ __forceinline__ void s3q_task(const FactorJobDev& J, const float* const* segs, int local,
                                         char* lds) {
  const int T3 = (J.n + MT - 1) / MT, units = T3 * (T3 + 1) / 2;
  const int split = local / units, unit = local - split * units;
  int I, Jc;
  s3_decode(unit, T3, I, Jc);
  const int64_t s0 = (int64_t)split * J.chunk;
  const int64_t s1 = min(J.nst, s0 + J.chunk);
  const int nh = 2 * (int)(s1 - s0);  // 16-row substeps (even)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  bool act[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const int r0 = I * MT + wr * 64 + bi * 32, c0 = Jc * MT + wc * 64 + bj * 32;
      act[bi][bj] = r0 < J.n && c0 < J.n && r0 >= c0;
    }
  floatx16 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[bi][bj][v] = 0.f;
  // this thread's column of the [A | B] panels
  const int ld4 = (int)J.x.ld * 4;
  const int rows = (int)J.x.rows;
  const int rec = rows * ld4;  // a batch's bytes (planner: < 2^31)
  const int gc = tid < MT ? I * MT + tid : Jc * MT + (tid - MT);
  const int voff = gc < J.x.cols ? gc * 4 : rec;  // past the operand: the zero tail
  const bool ones = gc == J.x.ones;
  const int wo = s3_half(tid, 0), wo1 = s3_half(tid, 1);
  // substep cursor: batch `seg` (base `b`), first row `k` of the substep within it
  const int sub_per_seg = 2 * J.sps;
  int seg = (int)(s0 / J.sps);
  int k = (int)((s0 - (int64_t)seg * J.sps) * BK);
  const int lastseg = J.nseg - 1;
  const float* b = seg_base(J, segs, seg);
  const float* nb = seg_base(J, segs, min(seg + 1, lastseg));  // the next batch's base
  int left = nh - 1;  // substeps after the cursor's within the task (it stops at the last)
  int ksub = k / 16;  // substep index within the batch
  // branch-free (scalar selects): a branch here splits the loop body and the compiler
  // then copies the load register sets at the join
  auto advance = [&]() {
    const int more = left > 0;
    left -= more;
    ksub += more;
    k += 16 * more;
    const bool wrap = ksub == sub_per_seg;
    ksub = wrap ? 0 : ksub;
    k = wrap ? 0 : k;
    seg += wrap;
    b = wrap ? nb : b;
    nb = seg_base(J, segs, min(seg + 1, lastseg));
  };
  struct Sub {
    int seg, k;
  };
  auto load = [&](float (&L)[2][8]) {
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(b), 0, rec, 0x00020000);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 8; ++r)
        L[u][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, (k + 8 * u + r) * ld4, 0));
  };
  auto put1 = [&](float (&x)[8], int u, const Sub& sb, char* slot) {
    if constexpr (FILL) {  // the ones column: 1 on the batch's rows, 0 past them
      const int nvalid = (int)seg_rows(J, sb.seg) - sb.k - 8 * u;
#pragma unroll
      for (int r = 0; r < 8; ++r) x[r] = ones ? (r < nvalid ? 1.f : 0.f) : x[r];
    }
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 hp, mp, lp;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t a2, b2, c2;
      split3(x[2 * i], x[2 * i + 1], a2, b2, c2);
      hp[i] = a2;
      mp[i] = b2;
      lp[i] = c2;
    }
    const int o = u ? wo1 : wo;
    *reinterpret_cast<u32x4*>(slot + o) = hp;
    *reinterpret_cast<u32x4*>(slot + S3_PART + o) = mp;
    *reinterpret_cast<u32x4*>(slot + 2 * S3_PART + o) = lp;
  };
  const int lo = s3_half(lane & 31, lane >> 5);
  const int oa = wr * 64 * 32 + lo, ob = (MT + wc * 64) * 32 + lo;
  auto frag = [&](const char* slot, int off) { return *reinterpret_cast<const bf16x8*>(slot + off); };
  float L0[2][8], L1[2][8];
  Sub sub0{seg, k}, sub1;
  load(L0);
  advance();
  sub1 = Sub{seg, k};
  load(L1);
  advance();
  asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // L0 landed
  put1(L0[0], 0, sub0, lds);
  put1(L0[1], 1, sub0, lds);
  __syncthreads();
  // substep hs: MFMAs from slot hs & 1; Lsplit (substep hs + 1) split into the other
  // slot during them; Lload refilled with substep hs + 2
  auto body = [&](int hs, float (&Lsplit)[2][8], const Sub& ssplit, float (&Lload)[2][8]) {
    const char* cur = lds + (hs & 1) * S3_REG;
    char* nxt = lds + ((hs + 1) & 1) * S3_REG;
    bf16x8 A[2][3], B[2][3];
#pragma unroll
    for (int p = 0; p < 3; ++p) A[0][p] = frag(cur, oa + p * S3_PART);
    load(Lload);  // (past the task's rows: the last substep again, never used)
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");  // Lsplit has landed
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      if (bi == 0)
#pragma unroll
        for (int p = 0; p < 3; ++p) A[1][p] = frag(cur, oa + p * S3_PART + 32 * 32);
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        if (bi == 0)
#pragma unroll
          for (int p = 0; p < 3; ++p) B[bj][p] = frag(cur, ob + p * S3_PART + bj * 32 * 32);
        const bf16x8* Aa = A[bi];
        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aa[2], B[bj][0], acc[bi][bj], 0, 0, 0);
        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aa[1], B[bj][1], acc[bi][bj], 0, 0, 0);
        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aa[0], B[bj][2], acc[bi][bj], 0, 0, 0);
        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aa[1], B[bj][0], acc[bi][bj], 0, 0, 0);
        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aa[0], B[bj][1], acc[bi][bj], 0, 0, 0);
        acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(Aa[0], B[bj][0], acc[bi][bj], 0, 0, 0);
      }
      // (unconditional: past the last substep it fills the free slot -- a branch here
      // made the compiler copy the 64 accumulators every trip)
      put1(Lsplit[bi], bi, ssplit, nxt);
      // pattern: the fragment reads first, then per MFMA ~4 VALU of the split, a DS
      // write every 4 MFMAs
      if (bi == 0) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (bi == 0 && i == 5) __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        if (i % 4 == 3) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  };
  for (int hs = 0; hs < nh; hs += 2) {
    const Sub s2{seg, k};
    body(hs, L1, sub1, L0);  // L0 <- substep hs + 2
    advance();
    sub0 = s2;
    const Sub s3{seg, k};
    body(hs + 1, L0, sub0, L1);  // L1 <- substep hs + 3
    advance();
    sub1 = s3;
  }
  const int ti = 2 * I + wr, tj = 2 * Jc + wc;
  float* o = J.slab + ((size_t)(ti * (ti + 1) / 2 + tj) * J.sstride + split) * TILE * TILE;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
      if (act[bi][bj])
        put_partial(J, acc[bi][bj],
                    [&](int v) { return &o[(bi * 32 + acc_row(v, lane)) * TILE + bj * 32 + (lane & 31)]; });
}

__global__ __launch_bounds__(NTHREADS, S3D_WGS) void kfac_factor_syrk3(FactorArgs args) {
  extern __shared__ __attribute__((aligned(16))) char s3lds[];
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int j = 0;
  while (j + 1 < args.njobs && task >= args.task_end[j]) ++j;
  const FactorJobDev& J = args.job[j];
  const int local = task - J.task_begin;
  if (J.n <= 32) {
    factor_task_narrow_direct(J, args.segs, local, reinterpret_cast<float*>(s3lds));
    return;
  }
  // the macro tile whose panels hold the ones column splits with the fill
  const int T3 = (J.n + MT - 1) / MT, units = T3 * (T3 + 1) / 2;
  int I, Jc;
  s3_decode(local % units, T3, I, Jc);
  const int o = J.x.ones;
  const bool fill = o >= 0 && (o / MT == I || o / MT == Jc);
  if (fill)
    s3q_task<true>(J, args.segs, local, s3lds);
  else
    s3q_task<false>(J, args.segs, local, s3lds);
}

// ------------------------------------------------------------------- host side
int64_t syrk3_units(int n) {
  const int64_t t3 = cdiv(n, MT);
  return n <= 32 ? 1 : t3 * (t3 + 1) / 2;
}

int launch_syrk3(const FactorArgs& args, int tasks, hipStream_t stream) {
  static const int lds = raise_dynamic_lds(reinterpret_cast<const void*>(&kfac_factor_syrk3), S3D_LDS);
  if (lds != KFAC_OK) return lds;
  hipLaunchKernelGGL(kfac_factor_syrk3, dim3(tasks), dim3(NTHREADS), S3D_LDS, stream, args);
  return KFAC_OK;
}

}  // namespace kfac
