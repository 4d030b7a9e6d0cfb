// The fp32-MFMA factor kernels and the reduce.
//   kfac_factor_tiles_t : grouped split-K fp32-MFMA SYRK.  A task is one 64x64
//      lower-triangle tile of one factor over one K-chunk; it writes a 64x64 fp32
//      partial slab (deterministic, no atomics).
//   kfac_factor_reduce  : per tile, sum the slabs in split order, apply
//      F = beta*F + alpha*sum, write the tile and its mirror (LDS transpose), so F stays
//      exactly symmetric.  Every family's slabs end here.
#include "factor_common.h"

namespace kfac {

template <int LAYOUT>
__device__ __forceinline__ void factor_task(const FactorJobDev& J, const float* const* segs, int local,
                                            float* lds) {
  // tile-major order: a tile's splits are consecutive tasks (one XCD; see the reduce)
  const int tile = local / J.splits, split = local - tile * J.splits;
  int ti, tj;
  tri_decode(tile, ti, tj);
  const int64_t s0 = (int64_t)split * J.chunk;
  const int64_t s1 = min(J.nst, s0 + J.chunk);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = wave >> 1, qj = wave & 1;
  const bool diag = ti == tj;
  // strictly-upper quadrant of a diagonal tile, or a quadrant wholly in the tile
  // padding (rows or columns >= n): no MFMA work (the reduce never reads it)
  const bool active = !(diag && qi < qj) && ti * TILE + qi * 32 < J.n && tj * TILE + qj * 32 < J.n;
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  const bool narrow = J.n <= 32;  // one 32x32 quadrant: the 4 waves split K instead
  if constexpr (LAYOUT == KFAC_ROWMAJOR) {
    // one pipelined contraction per batch piece of this split's stage range
    StageCursor c;
    c.init(J, s0);
    for (int64_t s = s0; s < s1;) {
      const int64_t here = min(s1 - s, (int64_t)J.sps - c.k / BK);
      contract_tile<LAYOUT, LAYOUT>(J.x, ti * TILE, J.x, tj * TILE, c.k,
                                    min(J.x.rows, c.k + here * BK), diag, active, lds, acc, narrow,
                                    seg_base(J, segs, c.seg));
      s += here;
      c.seg += 1;
      c.k = 0;
    }
  } else {
    // channel-major / im2col jobs are single-batch (validate()): stage s = rows [s*BK, ..)
    contract_tile<LAYOUT, LAYOUT>(J.x, ti * TILE, J.x, tj * TILE, s0 * BK, min(J.x.rows, s1 * BK),
                                  diag, active, lds, acc, narrow);
  }
  if (narrow) {
    store_narrow(J, J.slab + ((size_t)tile * J.sstride + split) * TILE * TILE, acc, lds);
    return;
  }
  if (!active) return;
  float* out = J.slab + ((size_t)tile * J.sstride + split) * TILE * TILE + qi * 32 * TILE + qj * 32;
  put_partial(J, acc, [&](int v) { return &out[acc_row(v, lane) * TILE + (lane & 31)]; });
}

// ---------------------------------------------------------------------------
// Row-major operands with 16-byte-aligned rows (cols, ld multiples of 4): panels
// arrive by LDS-DMA (global_load_lds_dwordx4) into a 3-slot ring, two stages in
// flight, counted vmcnt + raw s_barrier (one per stage), no staging VGPRs.  The
// image is lane-linear [32 rows][64 cols] (256-byte rows, unpadded: the MFMA's
// ds_read_b32 halves read 32 consecutive dwords, conflict-free).  Chunks past the
// last real column (bias ones column, tile padding) and rows past the range load
// from a safe address and are overwritten with their fill value once landed.
// GBK rows per stage; each thread of NW waves owns NCH = GBK/(4 NW) of a panel's
// 16-byte chunks.
template <int GBK, int NW = 4>
struct GldsPanel {
  static constexpr int NCH = GBK / (4 * NW);
  // chunk i of wave w, lane l: row (w NCH + i) * 4 + (l >> 4), columns col .. col + 3
  // with col = col0 + 4 (l & 15) -- the same columns for every chunk of the lane
  int64_t ld, kend;
  int col, ones, lrow;
  bool real;   // the lane's chunks hold matrix data (else fill: ones column -> 1)
  bool fillw;  // some lane of the wave has fill chunks
  __device__ __forceinline__ void init(const OpDev& op, int col0, int w, int lane, int64_t k_end) {
    ld = op.ld; kend = k_end;
    col = col0 + (lane & 15) * 4;
    real = col < op.cols;
    ones = op.ones;
    lrow = w * NCH * 4 + (lane >> 4);
    fillw = __ballot(!real) != 0;
  }
  // issue the LDS-DMA loads of rows [k, k+GBK) of the batch at `base` into `slot`
  __device__ __forceinline__ void issue(const float* base, int64_t k, float* slot, int w) const {
    if (k + GBK <= kend) {  // whole stage inside the batch: no row clamp
      const float* p = base + (k + lrow) * ld + (real ? col : 0);
#pragma unroll
      for (int i = 0; i < NCH; ++i)
        __builtin_amdgcn_global_load_lds(p + 4 * i * ld, slot + (w * NCH + i) * 256, 16, 0, 0);
      return;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int64_t row = k + lrow + 4 * i;
      const int64_t r = row < kend ? row : kend - 1;
      const float* src = base + r * ld + (real ? col : 0);
      __builtin_amdgcn_global_load_lds(src, slot + (w * NCH + i) * 256, 16, 0, 0);
    }
  }
  // after landing: overwrite chunks that must not hold matrix data (none: a whole
  // stage of real columns)
  __device__ __forceinline__ void fixup(int64_t k, float* slot) const {
    if (!fillw && k + GBK <= kend) return;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const bool okrow = k + lrow + 4 * i < kend;
      if (!real || !okrow) {
        // inline asm: the explicit vm_wait already covers this lane's DMA; a plain
        // store would make the compiler drain every in-flight stage (vmcnt(0))
        typedef float f4v __attribute__((ext_vector_type(4)));
        f4v v = {0.f, 0.f, 0.f, 0.f};
        if (okrow) {
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = col + q == ones ? 1.f : 0.f;
        }
        const uint32_t addr = (uint32_t)(uintptr_t)(slot + ((lrow / 4 + i) * 64 + lane) * 4);
        asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(v) : "memory");
      }
    }
  }
};

__device__ __forceinline__ void vm_wait(int n) {
  // counted waits need immediates: n = DMA instructions allowed to stay in flight
  switch (n) {
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 18: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    case 24: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

__device__ __forceinline__ void stage_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// NSLOT ring slots (2: one stage in flight, 4 WGs/CU); one barrier per stage.
template <int GBK, int NSLOT>
__device__ __forceinline__ void factor_task_glds(const FactorJobDev& J, const float* const* segs,
                                                 int local, float* lds, int split_major) {
  static_assert(NSLOT >= 2, "ring must hold the computed stage and the next one");
  // split-major order: xcd_task hands every XCD a contiguous range of K-splits of
  // ALL tiles, so each XCD streams ~1/8 of the operand rows through its L2 once
  // (tile-major gave every XCD all K of its tiles' panels: ~8x the HBM fetch on
  // the multi-batch launches of a queued pass)
  const int ntiles = J.t * (J.t + 1) / 2;
  const int split = split_major ? local / ntiles : local % J.splits;
  const int tile = split_major ? local - split * ntiles : local / J.splits;
  int ti, tj;
  tri_decode(tile, ti, tj);
  const int64_t s0 = (int64_t)split * J.chunk;
  const int64_t s1 = min(J.nst, s0 + J.chunk);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // quadrant of this wave, rotated per dispatch round: the ~4 workgroups sharing a CU
  // put their idle quadrants (strictly-upper on diagonal tiles, tile padding) on
  // different SIMDs instead of all on the same one
  const int qw = (wave + (int)(blockIdx.x >> 8)) & 3;
  const int qi = qw >> 1, qj = qw & 1;
  const bool same = ti == tj;
  const bool active = !(same && qi < qj) && ti * TILE + qi * 32 < J.n && tj * TILE + qj * 32 < J.n;
  const bool narrow = J.n <= 32;  // one 32x32 quadrant: the 4 waves split K instead
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;

  static_assert(GBK == BK, "a ring slot is one planner stage");
  if (s1 > s0) {
    // ring of NSLOT slots of GBK rows; NSLOT - 1 slots are in flight while a stage
    // computes.  Slots are issued and landed in stage order, each walked by its own
    // cursor across batch boundaries.
    constexpr int GSLOT = 2 * GBK * TILE;  // floats per ring slot (A and B panels)
    const int64_t rows = J.x.rows;
    GldsPanel<GBK> pa, pb;
    pa.init(J.x, ti * TILE, wave, lane, rows);
    pb.init(J.x, tj * TILE, wave, lane, rows);
    const int ns = (int)(s1 - s0);  // slots of this task
    const int per = (same ? 1 : 2) * GldsPanel<GBK>::NCH;  // LDS-DMA instructions per slot per thread
    StageCursor ic, fc;  // next slot to issue / to land
    ic.init(J, s0);
    fc = ic;
    const float* ibase = seg_base(J, segs, ic.seg);
    auto issue = [&](int sl) {
      float* slot = lds + (sl % NSLOT) * GSLOT;
      pa.issue(ibase, ic.k, slot, wave);
      if (!same) pb.issue(ibase, ic.k, slot + GBK * TILE, wave);
      const int seg = ic.seg;
      ic.next(rows);
      if (ic.seg != seg && sl + 1 < ns) ibase = seg_base(J, segs, ic.seg);
    };
#pragma unroll
    for (int p0 = 0; p0 < NSLOT - 1; ++p0)
      if (p0 < ns) issue(p0);
    const int h = lane >> 5, rr = lane & 31;
    for (int st = 0; st < ns; ++st) {
      // slot st landed; those issued after it may still fly
      const int issued = min(ns - 1, st + NSLOT - 2);
      vm_wait(per * (issued - st));
      float* slot = lds + (st % NSLOT) * GSLOT;
      pa.fixup(fc.k, slot);
      if (!same) pb.fixup(fc.k, slot + GBK * TILE);
      fc.next(rows);
      stage_barrier();  // stage st visible to all waves; everyone is done with stage st-1's slot
      if (st + NSLOT - 1 < ns) issue(st + NSLOT - 1);
      if (narrow) {
        const float* a = slot + h * TILE + rr;
#pragma unroll
        for (int s2 = 0; s2 < GBK / 8; ++s2) {
          const int ks = 2 * (wave * (GBK / 8) + s2);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks * TILE], a[ks * TILE], acc, 0, 0, 0);
        }
      } else if (active) {
        const float* a = slot + h * TILE + qi * 32 + rr;
        const float* b = slot + (same ? 0 : GBK * TILE) + h * TILE + qj * 32 + rr;
        float av[GBK / 2], bv[GBK / 2];
#pragma unroll
        for (int s2 = 0; s2 < GBK / 2; ++s2) {
          av[s2] = a[2 * s2 * TILE];
          bv[s2] = b[2 * s2 * TILE];
        }
#pragma unroll
        for (int s2 = 0; s2 < GBK / 2; ++s2)
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc, 0, 0, 0);
        // DS reads interleaved with the MFMAs (-1.2 us of 42 on the MLP update; a deeper
        // lookahead, the reads of MFMA pair t+2..4 issued with pair t, measured equal)
#pragma unroll
        for (int s2 = 0; s2 < GBK / 2; ++s2) {
          __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // 2 DS reads
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // 1 MFMA
        }
      }
    }
  }
  if (narrow) {  // (narrow => one tile, diagonal: A and B panels are the same)
    __syncthreads();
    store_narrow(J, J.slab + ((size_t)tile * J.sstride + split) * TILE * TILE, acc, lds);
    return;
  }
  if (!active) return;
  float* out = J.slab + ((size_t)tile * J.sstride + split) * TILE * TILE + qi * 32 * TILE + qj * 32;
  put_partial(J, acc, [&](int v) { return &out[acc_row(v, lane) * TILE + (lane & 31)]; });
}


// One launch per grouped update.  The row-major family (FAMILY = KFAC_ROWMAJOR)
// takes the LDS-DMA path when a job's operand allows it, else the register-staged
// row-major path; channel-major and im2col jobs get launches (and register budgets)
// of their own, instantiated per layout.  GLDS_ONLY: every job takes the LDS-DMA
// path (or the narrow direct-load path), and the ring is all the LDS (32 KB, not the
// register-staged path's 34 KB): 4 resident workgroups leave 32 KB of a CU's 160,
// room for a 32-tile inversion workgroup (29 KB) of an overlapped invert().
// Start delay per dispatch round (blockIdx / 256), in 512-cycle s_sleep(8) units: the
// workgroups that share a CU start ~1 us apart, so their load / barrier stalls
// interleave instead of coinciding (fp32 LDS-DMA SYRK: +2.5 %).  A design
// constant, not a timing build.
constexpr int STAGGER = 5;

template <int GBK, int NSLOT, bool GLDS_ONLY = false, int FAMILY = KFAC_ROWMAJOR>
__global__ __launch_bounds__(NTHREADS, 4) void kfac_factor_tiles_t(FactorArgs args) {
  constexpr int RING = FAMILY == KFAC_ROWMAJOR ? NSLOT * 2 * GBK * TILE : 0;
  constexpr int LDSF = GLDS_ONLY ? RING : ((4 * PANEL > RING) ? 4 * PANEL : RING);
  __shared__ __attribute__((aligned(16))) float lds[LDSF];
  // Workgroups of later dispatch rounds (blockIdx / 256: the ~4 sharing a CU) start a
  // fraction of a stage later, so their DMA waits and barriers interleave instead of
  // stalling all 16 waves of a CU together (measured +2.5% on the MLP update).
  for (int i = 0; i < STAGGER * (int)(blockIdx.x >> 8); ++i) __builtin_amdgcn_s_sleep(8);
  const int task = xcd_task(blockIdx.x, gridDim.x);
  int j = 0;
  while (j + 1 < args.njobs && task >= args.task_end[j]) ++j;
  const FactorJobDev& J = args.job[j];
  const int local = task - J.task_begin;
  if constexpr (FAMILY == KFAC_ROWMAJOR) {
    const float* const* segs = args.segs;
    if (J.glds)
      factor_task_glds<GBK, NSLOT>(J, segs, local, lds, args.split_major);
    else if constexpr (GLDS_ONLY)
      factor_task_narrow_direct(J, segs, local, lds);
    else
      factor_task<KFAC_ROWMAJOR>(J, segs, local, lds);
  } else {
    factor_task<FAMILY>(J, nullptr, local, lds);
  }
}

// production configuration: 32-row stages, 2-slot ring (one stage in flight)
#define kfac_factor_tiles kfac_factor_tiles_t<32, 2>
#define kfac_factor_tiles_glds kfac_factor_tiles_t<32, 2, true>
#define kfac_factor_tiles_channel kfac_factor_tiles_t<32, 2, false, KFAC_CHANNEL>
#define kfac_factor_tiles_patch kfac_factor_tiles_t<32, 2, false, KFAC_PATCH>

// One block = one 4-row strip of one 64x64 tile.  Each float4 of the strip is
// summed by 4 threads over interleaved splits (part p: splits p, p+4, ...); the
// partials combine in LDS in part order (deterministic; no atomics), then
// F = beta*F + alpha*sum and the mirrored upper element (same value: F stays
// exactly symmetric).  16 blocks per tile keep jobs with one tile and many splits
// (narrow conv factors: ~1000 slabs) parallel.
constexpr int RSTRIP = 4;  // rows per reduce block

__global__ __launch_bounds__(NTHREADS) void kfac_factor_reduce(FactorArgs args) {
  __shared__ float4 part_sum[4][64];
  __shared__ float tot[RSTRIP][TILE + 1];
  // same proportional XCD mapping as the tiles launch: a tile's strips run on the XCD
  // whose L2 holds its freshly written slabs
  const int rb = xcd_task(blockIdx.x, gridDim.x);
  const int gtile = rb / (TILE / RSTRIP), s0 = (rb % (TILE / RSTRIP)) * RSTRIP;
  int j = 0;
  while (j + 1 < args.njobs && gtile >= args.tile_end[j]) ++j;
  const FactorJobDev& J = args.job[j];
  const int tile = gtile - J.tile_begin;
  int ti, tj;
  tri_decode(tile, ti, tj);
  const int i0 = ti * TILE, j0 = tj * TILE, n = J.n;
  const bool diag = ti == tj;
  const int part = threadIdx.x >> 6, f = threadIdx.x & 63;  // f: float4 of the 4 x 64 strip
  const int r = f >> 4, c4 = (f & 15) * 4;
  const float4* slab =
      reinterpret_cast<const float4*>(J.slab + (size_t)tile * J.sstride * TILE * TILE) +
      (((s0 + r) * TILE + c4) >> 2);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  const int S = J.splits;
  int sp = part;
  for (; sp + 12 < S; sp += 16) {  // four splits of this part in flight
    const float4 a = slab[(size_t)(sp + 0) * (TILE * TILE / 4)];
    const float4 b = slab[(size_t)(sp + 4) * (TILE * TILE / 4)];
    const float4 c = slab[(size_t)(sp + 8) * (TILE * TILE / 4)];
    const float4 d = slab[(size_t)(sp + 12) * (TILE * TILE / 4)];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
    acc.x += c.x; acc.y += c.y; acc.z += c.z; acc.w += c.w;
    acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
  }
  for (; sp < S; sp += 4) {
    const float4 a = slab[(size_t)sp * (TILE * TILE / 4)];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
  }
  part_sum[part][f] = acc;
  __syncthreads();
  if (part == 0) {
    float4 t = part_sum[0][f];
#pragma unroll
    for (int p = 1; p < 4; ++p) {
      const float4 u = part_sum[p][f];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    const float sum[4] = {t.x, t.y, t.z, t.w};
    const int gi = i0 + s0 + r;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c4 + q, gj = j0 + c;
      float val = 0.f;
      if (gi < n && gj < n && !(diag && c > s0 + r)) {
        float* fp = J.F + (int64_t)gi * J.ldF + gj;
        val = J.beta == 0.f ? J.alpha * sum[q] : J.beta * (*fp) + J.alpha * sum[q];
        *fp = val;
      }
      tot[r][c] = val;
    }
  }
  __syncthreads();
  // mirror: F[j0 + c][i0 + s0 + rr] = tot[rr][c] (diag tiles: strictly-lower sources)
  const int c = threadIdx.x >> 2, rr = threadIdx.x & 3;
  const int si = i0 + s0 + rr, sj = j0 + c;
  if (si < n && sj < n && !(diag && c >= s0 + rr)) J.F[(int64_t)sj * J.ldF + si] = tot[rr][c];
}

// ------------------------------------------------------------------- host side
int launch_tiles(const FactorArgs& args, int tasks, hipStream_t stream) {
  switch (args.job[0].x.layout) {
    case KFAC_CHANNEL:
      hipLaunchKernelGGL(kfac_factor_tiles_channel, dim3(tasks), dim3(NTHREADS), 0, stream, args);
      break;
    case KFAC_PATCH:
      hipLaunchKernelGGL(kfac_factor_tiles_patch, dim3(tasks), dim3(NTHREADS), 0, stream, args);
      break;
    default: {
      bool all_glds = true;
      for (int i = 0; i < args.njobs; ++i) all_glds &= args.job[i].glds != 0 || args.job[i].n <= 32;
      if (all_glds)
        hipLaunchKernelGGL(kfac_factor_tiles_glds, dim3(tasks), dim3(NTHREADS), 0, stream, args);
      else
        hipLaunchKernelGGL(kfac_factor_tiles, dim3(tasks), dim3(NTHREADS), 0, stream, args);
    }
  }
  return KFAC_OK;
}

// One reduce launch over the jobs of `red`, whose slabs are described by slab / splits.
void launch_reduce(const FactorArgs& red, int tiles, hipStream_t stream) {
  if (tiles == 0) return;
  ProfScope ps(KFAC_PROF_FACTOR_REDUCE, stream);
  hipLaunchKernelGGL(kfac_factor_reduce, dim3(tiles * (TILE / RSTRIP)), dim3(NTHREADS), 0, stream,
                     red);
}

}  // namespace kfac
