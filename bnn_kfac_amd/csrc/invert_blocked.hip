// The blocked path of the fp64 inversion (invert.hip): 64x64 tiles, some factor larger
// than 1536 (T >= 25 tiles per edge).  Throughput-bound: the panel of a step is formed
// once (inv_panel), and the updates are applied per block of PANEL_BLOCK panels, the
// bulk of a block's update running beside the next block's chain (look-ahead).
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "kfac_common.h"

namespace kfac {
namespace t64 {
constexpr int NB = 64;
#include "invert_tiles.inc"

// build R' (one tile per workgroup), Z = 0, info = 0
__global__ __launch_bounds__(NTHREADS) void inv_build(InvArgs args) {
  __shared__ float P[NB * (NB + 1)];  // P[a][b] = F[fi(a)][fc(b)]
  __shared__ float Q[NB * (NB + 1)];  // Q[b][a] = F[fc(b)][fi(a)]
  const int j = find_job(args, blockIdx.x);
  const InvJobDev& J = args.job[j];
  const int local = blockIdx.x - args.begin[j];
  if (local == 0 && threadIdx.x == 0 && J.info) *J.info = 0;
  int ti, tj;
  tri_decode(local, ti, tj);
  build_tile(J, ti, tj, P, Q, nullptr);
}

// -------------------------------------------------------------------- panel k
// Formed ONCE per step, C in place in W and the final X[k][j] in place in X (the
// merged path's per-workgroup panel recomputation would triple the trailing GEMM
// work at this many tiles per edge).  Final X stays entirely in X.
__global__ __launch_bounds__(NTHREADS) void inv_panel(InvArgs args) {
  __shared__ __attribute__((aligned(16))) double A[NB * DP];
  __shared__ __attribute__((aligned(16))) double Xk[NB * DP];
  const int jb = find_job(args, blockIdx.x);
  const InvJobDev& J = args.job[jb];
  const int k = args.step, T = J.T;
  const int local = blockIdx.x - args.begin[jb];
  const int nC = T - k - 1;
  doublex4 acc[BPW];
  if (local < nC) {  // C[i][k] = R'[i][k] X[k][k]^T
    const int i = k + 1 + local;
    double* t = tile_ptr(J.W, J.Np, i, k);
    load_tiles(Xk, tile_ptr(J.X, J.Np, k, k), A, t, nullptr, nullptr, J.Np);
    __syncthreads();
    gemm64<true>(A, Xk, acc);
    store_acc_global(t, J.Np, acc, 1.0, false);
  } else {           // X[k][j] = X[k][k] Z[k][j]
    const int j = local - nC;
    double* t = tile_ptr(J.X, J.Np, k, j);
    load_tiles(Xk, tile_ptr(J.X, J.Np, k, k), A, t, nullptr, nullptr, J.Np);
    __syncthreads();
    gemm64<false>(Xk, A, acc);
    store_acc_global(t, J.Np, acc, 1.0, false);
  }
}

// ------------------------------------------------------------ blocked updates
// Applying every panel on its own re-reads and rewrites the whole trailing matrix (and
// the Z region) once per panel: for a 4097^2 factor (65 panels of 64) that traffic, not
// the fp64 MFMA work, sets the time.  With panel blocks of PB panels [k0, ke):
//   per panel k in the block: inv_panel(k), then inv_inner(k) -- the updates the
//     block's later panels need: trailing tiles in the block's columns (i >= j,
//     k < j < ke) and Z tiles in the block's rows (k < i < ke, j <= k); the
//     (k+1, k+1) workgroup factors it (k + 1 < ke);
//   then ONE inv_bulk(k0, ke): every other trailing tile (i >= j >= ke) takes all PB
//     panels at once, R'[i][j] -= sum_k C[i][k] C[j][k]^T, and every Z tile of the
//     rows below (i >= ke, j < ke) Z[i][j] -= sum_{k >= j} C[i][k] X[k][j]; inv_diag
//     then factors the (ke, ke) tile.
// A tile is then read-modified-written once per block instead of once per panel
// (same arithmetic, summed in another order).
__device__ __forceinline__ void gemm64_acc_nt(const double* A, const double* B, doublex4 (&acc)[BPW]) {
#pragma unroll
  for (int x = 0; x < BPW; ++x)
    mfma_block<true>(A + 16 * blk_r(x) * DP, DP, B + 16 * blk_c(x) * DP, DP, NB, acc[x]);
}
__device__ __forceinline__ void gemm64_acc_nn(const double* A, const double* B, doublex4 (&acc)[BPW]) {
#pragma unroll
  for (int x = 0; x < BPW; ++x)
    mfma_block<false>(A + 16 * blk_r(x) * DP, DP, B + 16 * blk_c(x), DP, NB, acc[x]);
}

// trailing tile (i, j): R'[i][j] -= sum_{k in [k0, k1)} C[i][k] C[j][k]^T; the
// (fi, fi) workgroup (fi = i = j) then factors it.
__device__ __forceinline__ void blk_trailing(const InvJobDev& J, int i, int j, int k0, int k1, bool factor,
                                             double* A, double* B, double* Y, double* dg) {
  doublex4 acc[BPW];
#pragma unroll
  for (int x = 0; x < BPW; ++x) acc[x] = doublex4{0.0, 0.0, 0.0, 0.0};
  for (int k = k0; k < k1; ++k) {
    load_tiles(A, tile_ptr(J.W, J.Np, i, k), B, tile_ptr(J.W, J.Np, j, k),
               (factor && k == k0) ? Y : nullptr, tile_ptr(J.W, J.Np, i, i), J.Np);
    __syncthreads();
    gemm64_acc_nt(A, i == j ? A : B, acc);
    __syncthreads();
  }
  if (!factor) {
    store_acc_global(tile_ptr(J.W, J.Np, i, j), J.Np, acc, -1.0, true);
    return;
  }
  if (k1 <= k0) {  // (no update: the diagonal tile as it stands)
    load_tile(Y, tile_ptr(J.W, J.Np, i, i), J.Np);
    __syncthreads();
  }
  const int col = threadIdx.x & 15;
#pragma unroll
  for (int x = 0; x < BPW; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) Y[(16 * blk_r(x) + acc_row64(v)) * DP + 16 * blk_c(x) + col] -= acc[x][v];
  __syncthreads();
  diag_factor(Y, A, dg);
  check_pivots(J, i, dg);
  store_tile(tile_ptr(J.X, J.Np, i, i), A, J.Np);
}

// Z tile (i, j): Z[i][j] -= sum_{k in [max(k0, j), k1)} C[i][k] X[k][j]  (X[k][j] is
// final for j < k, X[k][k] for j = k)
__device__ __forceinline__ void blk_z(const InvJobDev& J, int i, int j, int k0, int k1, double* A,
                                      double* B) {
  doublex4 acc[BPW];
#pragma unroll
  for (int x = 0; x < BPW; ++x) acc[x] = doublex4{0.0, 0.0, 0.0, 0.0};
  for (int k = max(k0, j); k < k1; ++k) {
    load_tiles(A, tile_ptr(J.W, J.Np, i, k), B, tile_ptr(J.X, J.Np, k, j), nullptr, nullptr, J.Np);
    __syncthreads();
    gemm64_acc_nn(A, B, acc);
    __syncthreads();
  }
  store_acc_global(tile_ptr(J.X, J.Np, i, j), J.Np, acc, -1.0, true);
}

// tasks of a job: inner update of panel k in block [.., ke) / bulk update of block [k0, ke)
__host__ __device__ inline int inner_trailing(int T, int k, int ke) {
  int c = 0;
  for (int j = k + 1; j < ke && j < T; ++j) c += T - j;
  return c;
}
__host__ __device__ inline int inner_tasks(int T, int k, int ke) {
  if (k >= T) return 0;
  const int e = ke < T ? ke : T;
  return inner_trailing(T, k, e) + (e > k + 1 ? (e - k - 1) * (k + 1) : 0);
}
__host__ __device__ inline int bulk_tasks(int T, int ke) {
  return ke >= T ? 0 : (T - ke) * (T - ke + 1) / 2 + (T - ke) * ke;
}
// look-ahead parts of a block's bulk update (e2 = end of the next block):
//   part 1: the next block's columns (trailing tiles i >= j, ke <= j < e2) and Z rows
//           (ke <= i < e2): what the next block's panels read;
//   part 2: the rest (trailing j >= e2, Z rows i >= e2), beside the next block's chain.
__host__ __device__ inline int bulk_next_trailing(int T, int ke, int e2) {
  int c = 0;
  for (int j = ke; j < e2; ++j) c += T - j;
  return c;
}
__host__ __device__ inline int bulk_part_tasks(int T, int ke, int e2, int part) {
  if (ke >= T) return 0;
  if (part == 0) return bulk_tasks(T, ke);
  e2 = e2 < T ? e2 : T;
  if (part == 1) return bulk_next_trailing(T, ke, e2) + (e2 - ke) * ke;
  return (T - e2) * (T - e2 + 1) / 2 + (T - e2) * ke;
}

__global__ __launch_bounds__(NTHREADS) void inv_inner(InvArgs args) {
  __shared__ __attribute__((aligned(16))) double A[NB * DP];
  __shared__ __attribute__((aligned(16))) double B[NB * DP];
  __shared__ __attribute__((aligned(16))) double Y[NB * DP];
  __shared__ double dg[NB + 352];
  const int jb = find_job(args, blockIdx.x);
  const InvJobDev& J = args.job[jb];
  const int k = args.step, T = J.T, ke = min(args.kend, T);
  int local = blockIdx.x - args.begin[jb];
  const int nT = inner_trailing(T, k, ke);
  if (local < nT) {  // column j in (k, ke), row i >= j
    int j = k + 1;
    while (local >= T - j) {
      local -= T - j;
      ++j;
    }
    const int i = j + local;
    blk_trailing(J, i, j, k, k + 1, i == k + 1 && j == k + 1, A, B, Y, dg);
    return;
  }
  const int u = local - nT;  // row i in (k, ke), column j <= k
  blk_z(J, k + 1 + u / (k + 1), u % (k + 1), k, k + 1, A, B);
}

// (two LDS tiles: 2 workgroups per CU; the (ke, ke) tile is stored like the others
// and factored by inv_diag right after)
__global__ __launch_bounds__(NTHREADS) void inv_bulk(InvArgs args) {
  __shared__ __attribute__((aligned(16))) double A[NB * DP];
  __shared__ __attribute__((aligned(16))) double B[NB * DP];
  const int jb = find_job(args, blockIdx.x);
  const InvJobDev& J = args.job[jb];
  const int k0 = args.step, T = J.T, ke = min(args.kend, T);
  int local = blockIdx.x - args.begin[jb];
  if (args.part == 1) {  // the next block's columns and Z rows
    const int e2 = min(args.ksplit, T);
    const int nT = bulk_next_trailing(T, ke, e2);
    if (local < nT) {
      int j = ke;
      while (local >= T - j) {
        local -= T - j;
        ++j;
      }
      blk_trailing(J, j + local, j, k0, ke, false, A, B, nullptr, nullptr);
      return;
    }
    const int u = local - nT;
    blk_z(J, ke + u / ke, u % ke, k0, ke, A, B);
    return;
  }
  const int r0 = args.part == 2 ? min(args.ksplit, T) : ke;  // first row / column
  const int nT = (T - r0) * (T - r0 + 1) / 2;
  if (local < nT) {
    int a, b;
    tri_decode(local, a, b);
    blk_trailing(J, r0 + a, r0 + b, k0, ke, false, A, B, nullptr, nullptr);
    return;
  }
  const int u = local - nT;
  blk_z(J, r0 + u / ke, u % ke, k0, ke, A, B);
}

// factor the diagonal tile (d, d) = (args.step, args.step) of every job: X[d][d]
__global__ __launch_bounds__(NTHREADS) void inv_diag(InvArgs args) {
  __shared__ __attribute__((aligned(16))) double A[NB * DP];
  __shared__ __attribute__((aligned(16))) double Y[NB * DP];
  __shared__ double dg[NB + 352];
  const InvJobDev& J = args.job[find_job(args, blockIdx.x)];
  const int d = args.step;
  load_tile(Y, tile_ptr(J.W, J.Np, d, d), J.Np);
  __syncthreads();
  diag_factor(Y, A, dg);
  check_pivots(J, d, dg);
  store_tile(tile_ptr(J.X, J.Np, d, d), A, J.Np);
}

// ---------------------------------------------------------------- host side
// Look-ahead (KFAC_INV_LOOKAHEAD, default 1): a block's bulk update is split into the
// part the next block's panels read (on the caller's stream) and the rest, which runs
// on a helper stream beside the next block's panel / inner chain (the latency-bound
// part of the step).  One helper stream and two ordering events per caller stream.
struct LookAhead {
  hipStream_t s = nullptr;  // the caller's stream
  hipStream_t s2 = nullptr;
  hipEvent_t chain = nullptr, rest = nullptr;
};
static std::mutex g_la_mu;
static std::vector<LookAhead> g_la;

constexpr size_t LA_MAX = 64;  // caller streams with a helper (stable addresses: reserved once)

static const LookAhead* look_ahead(hipStream_t s) {
  if (!knobs().inv_lookahead) return nullptr;
  std::lock_guard<std::mutex> lk(g_la_mu);
  for (const LookAhead& l : g_la)
    if (l.s == s) return &l;
  // past LA_MAX caller streams the blocked path runs without the helper (nothing created)
  g_la.reserve(LA_MAX);
  if (g_la.size() == LA_MAX) return nullptr;
  LookAhead l;
  l.s = s;
  if (hipStreamCreateWithFlags(&l.s2, hipStreamNonBlocking) != hipSuccess) return nullptr;
  if (hipEventCreateWithFlags(&l.chain, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&l.rest, hipEventDisableTiming) != hipSuccess) {
    if (l.chain) (void)hipEventDestroy(l.chain);
    (void)hipStreamDestroy(l.s2);
    return nullptr;
  }
  g_la.push_back(l);
  return &g_la.back();
}

void release_look_ahead() {
  std::lock_guard<std::mutex> lk(g_la_mu);
  for (LookAhead& l : g_la) {
    (void)hipStreamSynchronize(l.s2);
    (void)hipEventDestroy(l.chain);
    (void)hipEventDestroy(l.rest);
    (void)hipStreamDestroy(l.s2);
  }
  g_la.clear();
}

// panels per block: 6 with the look-ahead and 16-byte loads (4097^2: 6.18 vs 6.25 ms
// at 4, 6.31 at 8)
constexpr int PANEL_BLOCK = 6;

// Phase 0 = the launch that reads F (inv_build); phase 1 = everything after it.
int invert_group(const kfac_invert_job* jobs, int njobs, char* ws, int32_t* info, hipStream_t s,
                 int phase) {
  InvArgs args;
  const int Tmax = fill_args(args, jobs, njobs, ws, info, nullptr);
  args.tpw = 1;
  if (!phase) return launch(inv_build, args, [](const InvJobDev& d) { return d.T * (d.T + 1) / 2; }, s);
  int rc = launch(inv_diag, args, [](const InvJobDev&) { return 1; }, s);  // step 0: X[0][0]
  if (rc) return rc;
  const LookAhead* la = look_ahead(s);
  bool rest_pending = false;
  for (int k0 = 0; k0 < Tmax; k0 += PANEL_BLOCK) {
    const int ke = k0 + PANEL_BLOCK, e2 = ke + PANEL_BLOCK;
    args.kend = ke;
    for (int k = k0; k < ke && k < Tmax; ++k) {
      args.step = k;
      rc = launch(inv_panel, args, [k](const InvJobDev& d) { return k < d.T ? d.T - 1 : 0; }, s);
      if (rc) return rc;
      rc = launch(inv_inner, args, [k, ke](const InvJobDev& d) { return inner_tasks(d.T, k, ke); }, s);
      if (rc) return rc;
    }
    args.step = k0;
    if (la && ke < Tmax) {
      // the chain of this block is done: the rest of its bulk may start (helper)
      if (hipEventRecord(la->chain, s) != hipSuccess) return KFAC_ELAUNCH;
      // the previous block's rest wrote the columns the next part updates
      if (rest_pending && hipStreamWaitEvent(s, la->rest, 0) != hipSuccess) return KFAC_ELAUNCH;
      args.ksplit = e2;
      args.part = 1;
      rc = launch(inv_bulk, args, [ke, e2](const InvJobDev& d) { return bulk_part_tasks(d.T, ke, e2, 1); }, s);
      if (rc) return rc;
      if (hipStreamWaitEvent(la->s2, la->chain, 0) != hipSuccess) return KFAC_ELAUNCH;
      args.part = 2;
      rc = launch(inv_bulk, args, [ke, e2](const InvJobDev& d) { return bulk_part_tasks(d.T, ke, e2, 2); },
                  la->s2);
      if (rc) return rc;
      if (hipEventRecord(la->rest, la->s2) != hipSuccess) return KFAC_ELAUNCH;
      rest_pending = true;
      args.part = 0;
    } else {
      if (rest_pending && hipStreamWaitEvent(s, la->rest, 0) != hipSuccess) return KFAC_ELAUNCH;
      rest_pending = false;
      rc = launch(inv_bulk, args, [ke](const InvJobDev& d) { return bulk_tasks(d.T, ke); }, s);
      if (rc) return rc;
    }
    args.step = ke;
    rc = launch(inv_diag, args, [ke](const InvJobDev& d) { return ke < d.T ? 1 : 0; }, s);
    if (rc) return rc;
  }
  if (rest_pending && hipStreamWaitEvent(s, la->rest, 0) != hipSuccess) return KFAC_ELAUNCH;
  return launch_outputs(args, s);
}

}  // namespace t64
}  // namespace kfac
