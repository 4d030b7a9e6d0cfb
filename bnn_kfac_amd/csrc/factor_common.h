// Kronecker-factor accumulation, internal: what the factor kernels (one file per kernel
// family, factor_<family>.hip) and the host side (factor.hip) share -- the launch
// argument structs, the kernels' common epilogue / stage-walking helpers, and each
// family's host interface: its geometry (where it has one), its launcher and the facts
// the K-split planner needs about it.
#pragma once

#include <cstddef>

#include "kfac_common.h"

namespace kfac {

// factor jobs per launch.  The kernel arguments (measured kernarg_segment_size) are
// 4,744 B for the FactorArgs kernels and 5,608 B for those that take a ConvGeom too:
// 4,488 B of FactorArgs, 864 B of ConvGeom, 256 B of implicit arguments.
// (kfac_factor_tiles_x3 takes its unit tables too: 8,192 B of X3Units.)
constexpr int MAXJ = 16;
constexpr int KSEG = 64;  // batch base pointers per launch (multi-batch jobs; +512 B)

struct FactorJobDev {
  OpDev x;
  float alpha, beta;
  float* F;
  int64_t ldF;
  float* slab;       // this job's slabs: tiles*splits x 64 x 64
  int seg_off;       // multi-batch job: its batch bases are FactorArgs::segs[seg_off..] (else -1)
  int64_t chunk;     // BK-row stages per split
  int64_t nst;       // stages of the job: nseg * sps
  int sps, nseg;     // stages per batch (a stage never straddles two batches), batches
  int n, t, splits;  // factor edge, tiles per edge, K-splits
  int task_begin;    // first global task of this job
  int glds;          // row-major, 16-byte-aligned rows: LDS-DMA kernel
  int tile_begin;    // first global tile of this job (reduce launch)
  int accum;         // deferred reduction: `slab` is the caller's accumulator
  float sbeta;       // accumulator update: slab = sbeta*slab + alpha*partial
  int x3tab;         // kfac_factor_tiles_x3: first entry of this job's unit table in X3Units::u
  int sstride;       // slabs per tile of `slab` (a job's split s of tile t: t * sstride + s)
  int x3units;       // kfac_factor_tiles_x3: units (workgroups per K-split) of that table
  // ragged last batch (x.last_rows, kfac_factor_tiles_x3 / narrow tasks only): its first
  // stage `rstage` (-1: none); its rows weigh rows / last_rows = `rw` times the others'
  // (its own per-batch mean): a task crossing into it scales its sums by 1 / rw = `rinv`
  // at rstage, and every task ending in it scales by rw at the end
  int64_t rstage;
  float rw, rinv;
  int rdelta;        // rows - last_rows (0: no ragged batch)
};

struct FactorArgs {
  const float* segs[KSEG];  // batch bases of the multi-batch jobs (kernel arguments: no copy)
  int njobs;
  // task order: 1 split-major within each job, 0 tile-major (KFAC_SYRK_ORDER); 2
  // (kfac_factor_tiles_x3 only, every job at job[0].splits K-splits): split-major across
  // the whole launch (x3_task_decode)
  int split_major;
  int task_end[MAXJ];
  int tile_end[MAXJ];
  FactorJobDev job[MAXJ];
};

// Epilogue write of one lane's 16 partial-tile values (`at(v)` = address of value
// v): a plain slab store, or, for a deferred-reduction job, the accumulator update
// slab = sbeta*slab + alpha*partial (old values loaded together first).
template <class At>
__device__ __forceinline__ void put_partial(const FactorJobDev& J, const floatx16& acc, At at) {
  if (!J.accum) {
#pragma unroll
    for (int v = 0; v < 16; ++v) *at(v) = acc[v];
    return;
  }
  if (J.sbeta == 0.f) {
#pragma unroll
    for (int v = 0; v < 16; ++v) *at(v) = J.alpha * acc[v];
    return;
  }
  float old[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) old[v] = *at(v);
#pragma unroll
  for (int v = 0; v < 16; ++v) *at(v) = fmaf(J.sbeta, old[v], J.alpha * acc[v]);
}

// The same for the first nb of a wave's N blocks (`at(i, v)`: value v of block i), split
// in two so the old values of every block are loaded before the first store (one round
// trip to the slab instead of nb: the compiler keeps a block's loads behind the previous
// block's stores) and can be in flight across the caller's partial-sum exchange.
template <int N, class At>
__device__ __forceinline__ void load_partials(const FactorJobDev& J, int nb, float (&old)[N][16], At at) {
  if (!J.accum || J.sbeta == 0.f) return;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i >= nb) break;
#pragma unroll
    for (int v = 0; v < 16; ++v) old[i][v] = *at(i, v);
  }
}
template <int N, class At>
__device__ __forceinline__ void put_partials(const FactorJobDev& J, int nb, const floatx16 (&acc)[N],
                                             const float (&old)[N][16], At at) {
  const bool upd = J.accum && J.sbeta != 0.f;
  const float a = J.accum ? J.alpha : 1.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if (i >= nb) break;
#pragma unroll
    for (int v = 0; v < 16; ++v) *at(i, v) = upd ? fmaf(J.sbeta, old[i][v], a * acc[i][v]) : a * acc[i][v];
  }
}

// K is walked in BK-row stages; stage s of a job is rows [k, k + BK) of batch
// `seg` (s = seg * sps + k / BK), so a multi-batch job reads each batch in place.
// `segs` = FactorArgs::segs (kernel-argument memory; never null: a conditional
// null pointer here makes the compiler copy the whole argument block to scratch).
// Both candidates are loaded and the VALUES selected (a single-batch job reads segs[0],
// some job's base or null, and drops it): written as one conditional expression this is
// a select of two argument-block addresses, which -- see seg_rows -- can cost that copy
// too (kfac_factor_tiles_x3 with six unit kinds: 4.5 KB of scratch per lane, 231 VGPRs).
__device__ __forceinline__ const float* seg_base(const FactorJobDev& J, const float* const* segs,
                                                 int seg) {
  const float* queued = segs[max(J.seg_off, 0) + seg];
  const float* single = J.x.ptr;
  return J.seg_off >= 0 ? queued : single;
}

// rows of batch `seg` of a job (its ragged last batch: x.last_rows).  Arithmetic, not a
// select of two fields: a select of two argument-block addresses makes the compiler
// copy the whole FactorArgs to scratch (4.5 KB per lane)
__device__ __forceinline__ int64_t seg_rows(const FactorJobDev& J, int seg) {
  return J.x.rows - (int64_t)(seg == J.nseg - 1) * J.rdelta;
}

// the ragged last batch's weight on a task's partial sums (see FactorJobDev::rstage)
template <int NA>
__device__ __forceinline__ void scale_acc(floatx16 (&acc)[NA], float f) {
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[a][v] *= f;
}

struct StageCursor {
  int seg;
  int64_t k;  // first row of the stage within batch `seg`
  __device__ __forceinline__ void init(const FactorJobDev& J, int64_t s) {
    seg = (int)(s / J.sps);
    k = (s - (int64_t)seg * J.sps) * BK;
  }
  __device__ __forceinline__ void next(int64_t rows) {
    k += BK;
    if (k >= rows) { k = 0; ++seg; }
  }
};

// Narrow factors (n <= 32): the 4 waves hold partial sums of quadrant (0,0) over
// disjoint K subsets; sum them through LDS in wave order (deterministic) and store
// the quadrant.  `lds` is free (the caller's stage loop has ended with a barrier).
template <int NW = 4>
__device__ __forceinline__ void store_narrow(const FactorJobDev& J, float* out, floatx16& acc,
                                             float* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < 16; ++v) lds[((wave - 1) * 16 + v) * 64 + lane] = acc[v];
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < NW - 1; ++w)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] += lds[(w * 16 + v) * 64 + lane];
  put_partial(J, acc, [&](int v) { return &out[acc_row(v, lane) * TILE + (lane & 31)]; });
}

// Narrow row-major factors (n <= 32) whose rows are not 16-B aligned (the MLP's
// 10-wide output gradient): operands go from global memory straight into the MFMA
// registers, one stage ahead, so the glds-only launch (32 KB of LDS) takes them
// too.  Of NW waves, wave w takes rows (BK/NW) w .. of every 32-row stage (the waves
// split K; the store sums them), lane (rr, h) row 2*s2 + h, column rr (the ones
// column: 1).
template <int NW = 4>
__device__ __forceinline__ void narrow_direct_load(const FactorJobDev& J, const float* base, int64_t k0,
                                                   int64_t rows, float (&v)[BK / (2 * NW)]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rr = lane & 31, h = lane >> 5;
#pragma unroll
  for (int s2 = 0; s2 < BK / (2 * NW); ++s2) {
    const int64_t k = k0 + 2 * (wave * (BK / (2 * NW)) + s2) + h;
    v[s2] = k < rows ? (rr < J.x.cols ? base[k * J.x.ld + rr] : (rr == J.x.ones ? 1.f : 0.f)) : 0.f;
  }
}

template <int NW = 4>
__device__ __forceinline__ void factor_task_narrow_direct(const FactorJobDev& J, const float* const* segs,
                                                          int local, float* lds) {
  constexpr int NV = BK / (2 * NW);
  const int split = local;  // one tile
  const int64_t s0 = (int64_t)split * J.chunk;
  const int64_t s1 = min(J.nst, s0 + J.chunk);
  floatx16 acc[1];
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[0][v] = 0.f;
  if (s1 > s0) {
    StageCursor c;
    c.init(J, s0);
    const float* base = seg_base(J, segs, c.seg);
    float cur[NV], nxt[NV];
    narrow_direct_load<NW>(J, base, c.k, seg_rows(J, c.seg), cur);
    for (int64_t s = s0; s < s1; ++s) {
      const int seg = c.seg;
      c.next(J.x.rows);
      if (s + 1 < s1) {
        if (c.seg != seg) base = seg_base(J, segs, c.seg);
        narrow_direct_load<NW>(J, base, c.k, seg_rows(J, c.seg), nxt);
      }
      if (s == J.rstage && s > s0) scale_acc(acc, J.rinv);  // (wave-uniform)
#pragma unroll
      for (int s2 = 0; s2 < NV; ++s2)
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[s2], cur[s2], acc[0], 0, 0, 0);
#pragma unroll
      for (int s2 = 0; s2 < NV; ++s2) cur[s2] = nxt[s2];
    }
    if (J.rstage >= 0 && s1 > J.rstage) scale_acc(acc, J.rw);
  }
  store_narrow<NW>(J, J.slab + (size_t)split * TILE * TILE, acc[0], lds);
}

// ------------------------------------------------------------ conv operands
// Geometry of a conv job (PATCH / CHANNEL operand) on a kernel whose tasks own whole
// images: the second kernel argument of every conv family.  Which family a job gets is
// the host's routing decision (factor.hip, route_group), not a field of this struct.
constexpr int CONV_SRC_MAX = 2048;  // per-image staged elements (PATCH) / float4s (CHANNEL)

typedef float floatx4 __attribute__((ext_vector_type(4)));

// kfac_factor_conv's block shape, by factor order (ConvGeom::mode; the kernel reads it)
enum ConvMode {
  CONV_BLOCKS = 0,  // n > 32: the lower triangle in 32x32 blocks, CONV_CB per wave
  CONV_N16 = 2,     // n <= 16: one 16x16 block
  CONV_N32 = 3,     // n in 17..32: three 16x16 blocks (1, one 32x32 block, was the A/B alternative)
};

struct ConvGeom {
  int mode;        // ConvMode (kfac_factor_conv only)
  int n;           // factor order
  int KR;          // k-lanes per MFMA (2 or 4)
  int B;           // images of the job: nseg batches x bseg images
  int bseg;        // images per batch (a multi-batch job walks the queued batches' bases)
  int T;           // MFMAs along one row group (PATCH: Wo; CHANNEL: segment length Q)
  int G;           // row groups (PATCH: ceil(Ho / KR)); CHANNEL: 1
  int stride;      // LDS step between consecutive MFMAs (PATCH: sw; CHANNEL: 1)
  int rowstep;     // PATCH: sh * Wp (one output row); CHANNEL: Q (one segment)
  int Ho;          // PATCH: output rows
  int plane;       // PATCH: Hp * Wp; CHANNEL: Lp = segments * Q (channel pitch)
  int Wp;          // PATCH: padded row pitch
  int ones_base;   // LDS offset of the all-ones plane (PATCH bias column)
  int zero_base;   // LDS offset of the all-zero plane (tile padding, rows past Ho)
  int lds;         // floats of LDS (>= the narrow reduce's 3 x 16 x 64)
  int src;         // staged source elements (PATCH) / float4s (CHANNEL) per image
  int nq;          // CONV_BLOCKS: 32x32 blocks of the factor's lower triangle
  int units;       // workgroups per K-split (CONV_BLOCKS: ceil(nq / (4*CONV_CB)) block groups; else 1)
  // kfac_factor_conv_x3 (im2col operand split into bf16x3 in LDS)
  int nb;          // 32-blocks per factor edge (im2col rows padded to 32 nb)
  int L;           // output positions per image (Ho * Wo)
  int Wo, sh, sw;  // output row length, strides
  int LPC;         // positions per chunk (multiple of 16): an image is ceil(L / LPC) chunks
  int nch;         // chunks per image
  int pitch;       // bf16 elements per im2col row (LPC + 8: 16-byte reads conflict-free)
  int imgf;        // floats of one staged fp32 image (C padded planes)
  int ones;        // bias column (-1: none)
  int ldsb;        // bytes of dynamic LDS
  int kw;          // waves per block (nq <= 4: the block's k-steps interleaved over kw waves)
  // kfac_factor_conv_x3s (one 32 x 32 block from column-shifted image copies)
  int xs_ncopy;    // copies (C x kernel width), then the ones copy and the zero copy
  int xs_hp;       // rows per copy (padded image rows)
  int xs_pw;       // bf16 per copy row (>= 8 xs_g8)
  int xs_cs;       // bf16 per copy (>= xs_hp xs_pw)
  int xs_g8;       // 8-position groups per output row (ceil(Wo / 8): 1, 2, 4 or 8)
  int xs_grp;      // groups per image (Ho xs_g8, even); k-step t holds groups 2t, 2t + 1
  int xs_np;       // build slots per image (C xs_hp xs_wp2)
  int xs_wp2;      // build slots per padded row (ceil((W + 2 pw) / 2))
  // kfac_factor_conv_x3f (flattened column copies; xs_hp / xs_wp2 / xs_np too)
  int xf_nv;       // shifted variants per copy (8-byte fragment reads)
  int xf_vmap;     // kernel row ki's variant in bits 2ki .. 2ki+1
  int xf_one, xf_zero, xf_dummy;  // part byte offsets of the ones / zero copies, the dummy row
  int xf_nks;      // 16-position k-steps per image (ceil(L / 16))
  int xf_wave[4];  // multiplying wave w: pattern (bits 0-3) and F[q] (bits 4 + 3q ..)
  int xs_lb[32];   // block row m's fragment byte offset in a part (copy, row, column)
  int8_t xs_f[32]; // block row m's factor row / column (data, bias, padding rows n..31)
  // kfac_factor_conv_x3f: copy (c, kj, v)'s part byte offset (shift included) in the u16 at 16 c + 2 kj + v
  int xf_cb[128];
};

// ------------------------------------------------- the families' host interface
// launch_<family>(args, [geometry,] tasks, stream) enqueues the family's kernel over
// `tasks` workgroups and returns KFAC_OK, or KFAC_ELAUNCH -- with nothing launched --
// when the kernel's dynamic-LDS limit could not be raised.  <family>_geom(operand, g)
// completes g (n, ones, B and bseg are the router's) and returns false when the
// operand does not fit the kernel.  The *_WGS constants are the resident workgroups per
// CU the K-split planner counts on for a family.

// The dynamic-LDS limit of `kernel`, raised once per process (call it from a function-
// local static, one per kernel); the status every later launch of that kernel returns.
static inline int raise_dynamic_lds(const void* kernel, int bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess
             ? KFAC_OK : KFAC_ELAUNCH;
}

// factor_tiles.hip: kfac_factor_tiles_t (fp32 MFMA; row-major groups, and conv jobs whose
// images no staged kernel takes, by the layout of job 0) and kfac_factor_reduce
constexpr int TILES_WGS = 4;  // (32 KB of LDS each)
int launch_tiles(const FactorArgs& args, int tasks, hipStream_t stream);
void launch_reduce(const FactorArgs& red, int tiles, hipStream_t stream);

// factor_syrk3.hip: kfac_factor_syrk3, 128 x 128 macro tiles (n <= 32: one narrow task)
constexpr int S3D_WGS = 2;  // (49 KB of LDS each)
int64_t syrk3_units(int n);
int launch_syrk3(const FactorArgs& args, int tasks, hipStream_t stream);

// factor_tiles_x3.hip: kfac_factor_tiles_x3.  Its work units of a factor of n are panel
// cliques: the factor's P = ceil(n / 32) column panels of 32 are the vertices of a complete
// graph whose edge (p, q) is the 32 x 32 block (p, q), and a unit is a clique of up to four
// panels whose workgroup splits each panel's fragment once and multiplies every pair of
// them -- a K4 is 6 blocks on 4 splits where a 64 x 64 tile is 4 blocks on 4.  The table of
// a P is an exact partition of the lower triangle: every block p > q in exactly one unit,
// every diagonal block in exactly one -- K4, K3, K2, diagonal units (up to four panels'
// (p, p)) and the two mixed kinds below.
// P = 25 (the MNIST MLP's 785) is the Steiner system S(2, 4, 25): 50 K4 units, 200 fragment
// splits for its 300 off-diagonal blocks; other P are packed greedily in a fixed order.
// Two mixed kinds take the pairs the cliques leave single together with diagonal blocks
// (panel slots ascending, as in a clique): S3D3, four slots, the blocks (3, 0), (3, 1),
// (3, 2) of the hub slot 3 and the diagonal blocks of slots 0, 1, 2 -- a K4's six blocks
// on its four splits; P1D2, two slots, (1, 0), (0, 0) and (1, 1).  P = 5 (the MLP's 129)
// is a K4, an S3D3 and a P1D2.
// One 32-bit entry per unit: panel s in bits 6s .. 6s+5 (unused slots repeat the last
// panel), the number of panels in bits 24-26, bit 28 a diagonal unit, bits 29-30 a mixed
// kind (X3_MIX_*; 0: a clique or a diagonal unit).
constexpr int X3_WGS = 4;     // (of two waves -- 3 or 2 measured slower)
constexpr int X3_PMAX = 64;   // panels per edge the 6-bit panel fields hold (n <= 2048)
constexpr int X3_UCAP = 2048; // table entries one launch carries (8 KB of kernel arguments)
constexpr uint32_t X3_DIAG = 1u << 28;
constexpr int X3_MIX_S3D3 = 1, X3_MIX_P1D2 = 2;
struct X3Units {
  uint32_t u[X3_UCAP];
};
__host__ __device__ inline int x3_unit_np(uint32_t u) { return (int)(u >> 24) & 7; }
__host__ __device__ inline int x3_unit_panel(uint32_t u, int s) { return (int)(u >> (6 * s)) & 63; }
__host__ __device__ inline int x3_unit_mix(uint32_t u) { return (int)(u >> 29) & 3; }
static inline int x3_panels(int n) { return (n + 31) / 32; }
// The launch-wide split-major task order of kfac_factor_tiles_x3 (FactorArgs::split_major
// == 2: every job at `splits` K-splits): with U the launch's units per split (a narrow job
// is one unit), logical task t -- xcd_task of workgroup `block` of `blocks` = U splits --
// is split t / U and launch-wide unit t % U, the jobs' units in job order: unit_end[j] =
// the units of jobs 0 .. j (FactorArgs::task_end in this order; task_begin likewise).
// xcd_task hands every XCD a contiguous range of t: where 8 divides the splits, whole
// splits -- each operand row is then fetched into one L2 only, and every XCD gets the
// same mix of units.
__host__ __device__ __forceinline__ void x3_task_decode(const int* unit_end, int njobs, int splits,
                                                        int blocks, int block, int& job, int& unit, int& split) {
  const int U = blocks / splits;
  const int t = xcd_task(block, blocks);
  split = t / U;
  const int lu = t - split * U;
  job = 0;
  while (job + 1 < njobs && lu >= unit_end[job]) ++job;
  unit = lu - (job > 0 ? unit_end[job - 1] : 0);
}
// the unit table of P panels (2 <= P <= X3_PMAX; built once per P, then shared) -- K4 and
// S3D3 units first, then the diagonal units, K3, P1D2 and K2: the longest first
int x3_unit_table(int P, const uint32_t** table);
// units of a factor of n (n <= 32: the one narrow task)
int x3_units(int n);
// entries the distinct tables of a launch group's factors take (<= X3_UCAP to launch)
int x3_table_entries(const int* n, int njobs);
int launch_tiles_x3(const FactorArgs& args, int tasks, hipStream_t stream);

// factor_conv.hip: kfac_factor_conv (fp32 MFMA, images staged in LDS; PATCH and CHANNEL).
// Its geometry is also the staging contract of the two channel kernels below.
constexpr int KFAC_CONV_OCC = 4;  // (what the CONV_BLOCKS instances are compiled for; the narrow ones too)
bool conv_fp32_geom(const kfac_operand& o, ConvGeom& g);
int launch_conv(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream);

// factor_conv_x3.hip / _x3s.hip / _x3f.hip: the bf16x3 im2col kernels (PATCH), one
// 512-thread workgroup per CU each
constexpr int CONV_X3_WGS = 1;
bool conv_x3_geom(const kfac_operand& o, ConvGeom& g);
int launch_conv_x3(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream);
bool conv_x3s_geom(const kfac_operand& o, ConvGeom& g);
int launch_conv_x3s(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream);
bool conv_x3f_geom(const kfac_operand& o, ConvGeom& g);
int launch_conv_x3f(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream);

// factor_channel.hip: CHANNEL factors with n <= 8 (kfac_factor_channel_small) and with
// 8 < n <= 32 (kfac_factor_channel_x3), on conv_fp32_geom's geometry
constexpr int CHANNEL_WGS = 4;
bool channel_small(const ConvGeom& g);
bool channel_x3_geom(const kfac_operand& o, ConvGeom& g);
int launch_channel_x3(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream);
int launch_channel_small(const FactorArgs& args, const ConvGeom& g, int tasks, hipStream_t stream);

}  // namespace kfac
