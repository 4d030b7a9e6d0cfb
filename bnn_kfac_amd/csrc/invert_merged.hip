// The merged path of the fp64 inversion (invert.hip): 32x32 tiles, every factor at most
// 1536 (T <= 48 tiles per edge).  Latency-bound: ONE launch per elimination step with
// the panel folded in, the steps of an all-inverse-Cholesky group replayed from a cached
// hipGraph.
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "kfac_common.h"

namespace kfac {
namespace t32 {
constexpr int NB = 32;
#include "invert_tiles.inc"

// C_i = R'[i][k] X[k][k]^T into Sdst (Xkk already in LDS; Sdst holds R'[i][k] on entry)
__device__ __forceinline__ void panel_tile_lds(double* Sdst, const double* Xkk) {
  doublex4 acc[BPW];
  gemm64<true>(Sdst, Xkk, acc);
  __syncthreads();  // every wave done reading R'[i][k] before it is overwritten
  store_acc_lds(Sdst, acc);
  __syncthreads();
}

// ------------------------------------------------------------------- step k
// One launch per elimination step (the panel is folded in: every workgroup forms
// the panel blocks it needs, C[i][k] = R'[i][k] X[k][k]^T, itself; C is never
// stored — column k is dead after step k).
//   k = -1        : build R'; task 0 factors tile (0,0)    -> X[0][0]
//   k <= T-2      : trailing  R'[i][j] -= C_i C_j^T        (i >= j > k)
//                   the (k+1,k+1) workgroup then factors   -> X[k+1][k+1]
//                   Z[i][j] -= C_i B,  B = X[k][k] (j = k) or X[k][k] Z[k][j] (j < k)
//                   row k+1's Z workgroups also store X[k][j] = X[k][k] Z[k][j]
//                   (final) into W[k][j], dead since step j (Z[k][j] stays intact
//                   for the other readers of this launch)
//   k = T-1       : X[k][j] = X[k][k] Z[k][j] -> W[k][j]   (j < k)
// Final inverse X: diagonal tiles in X, strictly-lower tiles in W (x_tile()).
// trailing tile (i, j), i >= j > k: R'[i][j] -= C_i C_j^T.  Returns true for the
// (k+1, k+1) workgroup, which then holds the updated diagonal tile in S2.
__device__ __forceinline__ bool step_trailing_ij(const InvJobDev& J, int k, int i, int j, double* S0,
                                                 double* S1, double* S2) {
  const bool diag = i == k + 1 && j == k + 1;
  // the (k+1,k+1) workgroup also prefetches its diagonal tile into the idle S2
  load_tiles(S0, tile_ptr(J.X, J.Np, k, k), S1, tile_ptr(J.W, J.Np, i, k),
             (j != i || diag) ? S2 : nullptr, tile_ptr(J.W, J.Np, j != i ? j : i, j != i ? k : i), J.Np);
  __syncthreads();
  panel_tile_lds(S1, S0);              // C_i
  if (j != i) panel_tile_lds(S2, S0);  // C_j
  doublex4 acc[BPW];
  gemm64<true>(S1, j != i ? S2 : S1, acc);
  if (!diag) {
    store_acc_global(tile_ptr(J.W, J.Np, i, j), J.Np, acc, -1.0, true);
    return false;
  }
  // the updated diagonal tile is consumed right here (never written back)
  const int col = threadIdx.x & 15;
#pragma unroll
  for (int x = 0; x < BPW; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) S2[(16 * blk_r(x) + acc_row64(v)) * DP + 16 * blk_c(x) + col] -= acc[x][v];
  __syncthreads();
  return true;
}

__device__ __forceinline__ bool step_trailing(const InvJobDev& J, int k, int local, double* S0,
                                              double* S1, double* S2) {
  int a, b;
  tri_decode(local, a, b);
  return step_trailing_ij(J, k, k + 1 + a, k + 1 + b, S0, S1, S2);
}

// Z tile (i, j), i > k >= j: Z[i][j] -= C_i B, B = X[k][k] (j = k) or
// X[k][k] Z[k][j] (j < k; row k+1's workgroup also stores it as the final X[k][j]).
__device__ __forceinline__ void step_z_ij(const InvJobDev& J, int k, int i, int j, double* S0,
                                          double* S1, double* S2) {
  load_tiles(S0, tile_ptr(J.X, J.Np, k, k), S1, tile_ptr(J.W, J.Np, i, k), j < k ? S2 : nullptr,
             tile_ptr(J.X, J.Np, k, j), J.Np);
  __syncthreads();
  panel_tile_lds(S1, S0);  // C_i
  doublex4 acc[BPW];
  const double* Bm = S0;
  if (j < k) {
    gemm64<false>(S0, S2, acc);
    __syncthreads();
    store_acc_lds(S2, acc);
    if (i == k + 1 && J.xw) store_acc_global(tile_ptr(J.W, J.Np, k, j), J.Np, acc, 1.0, false);
    __syncthreads();
    Bm = S2;
  }
  gemm64<false>(S1, Bm, acc);
  store_acc_global(tile_ptr(J.X, J.Np, i, j), J.Np, acc, -1.0, true);
  if (j < k && i == k + 1 && J.fout) emit_out(J, k, j, S2);  // final X[k][j]
}

__device__ __forceinline__ void step_z(const InvJobDev& J, int k, int u, double* S0, double* S1,
                                       double* S2) {
  step_z_ij(J, k, k + 1 + u / (k + 1), u % (k + 1), S0, S1, S2);
}

// The second task of a workgroup when it is in the same row i as the first one (tpw = 2
// takes consecutive tasks): S0 still holds X[k][k] and S1 the panel block C_i, so only
// the other operand is loaded and only its panel block formed (two of the three tile
// loads and one of the three panel / update GEMMs of a trailing task saved).
__device__ __forceinline__ void step_trailing_next(const InvJobDev& J, int k, int i, int j, double* S0,
                                                   double* S1, double* S2) {
  if (j != i) {
    load_tile(S2, tile_ptr(J.W, J.Np, j, k), J.Np);
    __syncthreads();
    panel_tile_lds(S2, S0);  // C_j
  }
  doublex4 acc[BPW];
  gemm64<true>(S1, j != i ? S2 : S1, acc);
  store_acc_global(tile_ptr(J.W, J.Np, i, j), J.Np, acc, -1.0, true);
}

__device__ __forceinline__ void step_z_next(const InvJobDev& J, int k, int i, int j, double* S0, double* S1,
                                            double* S2) {
  doublex4 acc[BPW];
  const double* Bm = S0;
  if (j < k) {
    load_tile(S2, tile_ptr(J.X, J.Np, k, j), J.Np);
    __syncthreads();
    gemm64<false>(S0, S2, acc);
    __syncthreads();
    store_acc_lds(S2, acc);
    if (i == k + 1 && J.xw) store_acc_global(tile_ptr(J.W, J.Np, k, j), J.Np, acc, 1.0, false);
    __syncthreads();
    Bm = S2;
  }
  gemm64<false>(S1, Bm, acc);
  store_acc_global(tile_ptr(J.X, J.Np, i, j), J.Np, acc, -1.0, true);
  if (j < k && i == k + 1 && J.fout) emit_out(J, k, j, S2);  // final X[k][j]
}

// (row, kind) of merged-step task `local` (k >= 0, k + 1 < T): kind 0 trailing, 1 Z
__device__ __forceinline__ void step_task_row(int T, int k, int local, int& i, int& j, int& kind) {
  const int nTrail = (T - k - 1) * (T - k) / 2;
  if (local < nTrail) {
    int a, b;
    tri_decode(local, a, b);
    i = k + 1 + a;
    j = k + 1 + b;
    kind = 0;
  } else {
    const int u = local - nTrail;
    i = k + 1 + u / (k + 1);
    j = u % (k + 1);
    kind = 1;
  }
}

// last row of X (k = T-1): X[k][j] = X[k][k] Z[k][j] -> W[k][j]
__device__ __forceinline__ void step_last_row(const InvJobDev& J, int k, int j, double* S0,
                                              double* S1) {
  load_tiles(S0, tile_ptr(J.X, J.Np, k, k), S1, tile_ptr(J.X, J.Np, k, j), nullptr, nullptr, J.Np);
  __syncthreads();
  doublex4 acc[BPW];
  gemm64<false>(S0, S1, acc);
  if (J.xw) store_acc_global(tile_ptr(J.W, J.Np, k, j), J.Np, acc, 1.0, false);
  if (J.fout) {
    __syncthreads();  // S1 fully read by the GEMM
    store_acc_lds(S1, acc);
    __syncthreads();
    emit_out(J, k, j, S1);
  }
}

// tasks of a job in step k: the build's tiles (k = -1), trailing + Z tiles, or the last
// row of X (k = T-1)
__host__ __device__ __forceinline__ int step_tasks(int T, int k) {
  if (k < 0) return T * (T + 1) / 2;
  if (k + 1 < T) return (T - k - 1) * (T - k) / 2 + (T - k - 1) * (k + 1);
  return k + 1 == T ? k : 0;
}

// workgroups of a job with `count` tasks.  tpw = 2: workgroup 0 takes the critical task
// alone, workgroup w >= 1 two tasks (see inv_step), so a step of a big factor fits one
// dispatch round beside a running SYRK launch (one 29 KB inversion workgroup per CU)
__host__ __device__ __forceinline__ int step_wgs(int count, int tpw) {
  return (tpw == 2 && count > 1) ? 1 + (count - 1 + 1) / 2 : count;
}

// one task of step k (task 0 of a job is its critical one: the build's tile
// (0,0) + its factorisation, or the trailing update + factorisation of (k+1, k+1))
__device__ __forceinline__ void step_task(const InvArgs& args, int jb, int local, double* S0, double* S1,
                                          double* S2, double* dg) {
  const InvJobDev& J = args.job[jb];
  const int k = args.step, T = J.T;
  const int nTrail = (T - k - 1) * (T - k) / 2;
  if (k < 0) {  // build R' (one tile per task); task 0 also factors tile (0,0)
    int ti, tj;
    tri_decode(local, ti, tj);
    if (local == 0 && threadIdx.x == 0 && J.info) *J.info = 0;
    build_tile(J, ti, tj, reinterpret_cast<float*>(S0), reinterpret_cast<float*>(S1),
               local == 0 ? S2 : nullptr);
    if (J.fout && ti != tj) emit_zero_block(J, ti, tj);
    if (local != 0) return;
    __syncthreads();
  } else if (k == T - 1) {
    step_last_row(J, k, local, S0, S1);
    if (J.fout && local == 0) emit_out(J, k, k, S0);  // emit_diag: the last diagonal block
    return;
  } else if (local >= nTrail) {
    step_z(J, k, local - nTrail, S0, S1, S2);
    if (J.fout && local == 1) emit_out(J, k, k, S0);  // emit_diag (S0 = X[k][k], intact)
    return;
  } else if (!step_trailing(J, k, local, S0, S1, S2)) {
    if (J.fout && local == 1) emit_out(J, k, k, S0);  // emit_diag (S0 = X[k][k], intact)
    return;
  }
  // the one diagonal factorisation of this step
  const int d = k + 1;
  diag_factor(S2, S1, dg);
  check_pivots(J, d, dg);
  store_tile(tile_ptr(J.X, J.Np, d, d), S1, J.Np);
  // its L block: emitted here only when no later step has a task to do it (T = 1);
  // otherwise a non-critical task of step d writes it from its own copy (emit_diag),
  // off this chain
  if (J.fout && T == 1) emit_out(J, d, d, S1);
}

__global__ __launch_bounds__(NTHREADS) void inv_step(InvArgs args) {
  // (no s_setprio: priority 3 made the chain win the SIMD's issue arbitration over a
  // running SYRK launch's waves; with a step of slack priority 0 measured +1-3 % on the
  // MLP line, the inversion stretching and the SYRK beside it running faster)
  __shared__ __attribute__((aligned(16))) double S0[NB * DP];
  __shared__ __attribute__((aligned(16))) double S1[NB * DP];
  __shared__ __attribute__((aligned(16))) double S2[NB * DP];
  __shared__ double dg[NB + 352];  // pivots + elimination broadcast buffers
  const int jb = find_job(args, blockIdx.x);
  const int wg = blockIdx.x - args.begin[jb];
  const int count = step_tasks(args.job[jb].T, args.step);
  // tpw = 2: workgroup w >= 1 takes the consecutive tasks 2w - 1 and 2w, which share
  // their row (and its panel block) unless a row boundary falls between them
  const int first = (args.tpw == 2 && wg >= 1) ? 2 * wg - 1 : wg;
  step_task(args, jb, first, S0, S1, S2, dg);
  const int second = first + 1;
  if (args.tpw == 2 && wg >= 1 && second < count) {
    __syncthreads();  // LDS tiles of the first task are read out
    const InvJobDev& J = args.job[jb];
    const int k = args.step, T = J.T;
    int i0 = -1, j0 = 0, kind0 = -1, i1 = -2, j1 = 0, kind1 = -2;
    if (k >= 0 && k + 1 < T) {
      step_task_row(T, k, first, i0, j0, kind0);
      step_task_row(T, k, second, i1, j1, kind1);
    }
    if (i0 == i1 && kind0 == kind1 && !(kind0 == 0 && i0 == k + 1 && j0 == k + 1)) {
      if (kind1 == 0) step_trailing_next(J, k, i1, j1, S0, S1, S2);
      else step_z_next(J, k, i1, j1, S0, S1, S2);
    } else {
      step_task(args, jb, second, S0, S1, S2, dg);
    }
  }
}

// ---------------------------------------------------------------- host side
// the arguments of step k's launch: `a` with step k and its job offsets; 0 = no tasks
static int step_args(InvArgs& a, int k) {
  a.step = k;
  int total = 0;
  for (int j = 0; j < a.njobs; ++j) {
    a.begin[j] = total;
    total += step_wgs(step_tasks(a.job[j].T, k), a.tpw);
  }
  a.begin[a.njobs] = total;
  return total;
}

static int launch_step(InvArgs& args, int k, hipStream_t s) {
  const int total = step_args(args, k);
  if (total == 0) return KFAC_OK;
  hipLaunchKernelGGL(inv_step, dim3(total), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// ------------------------------------------------------- graph-replayed step chain
// The latency-bound inversion is ~25 dependent step launches; issuing them costs
// the host more than the GPU spends per step.  With KFAC_INV_GRAPH (default on) the
// steps are one cached hipGraph per (stream, job set): the launches' arguments must
// then not change between calls, so every step writes L and the verdict to staging
// buffers in the workspace, and one inv_copy_out launch after the graph copies them
// to the caller's outputs.  The graph is rebuilt when anything else in the
// arguments changes (factor pointers, sizes, damping, workspace).
struct UnstageJob {
  const float* src;
  float* dst;
  int64_t ldo;
  const int* isrc;
  int* idst;
  int n;
};
struct UnstageArgs {
  int njobs;
  int begin[IMAXJ + 1];  // blocks per job: ceil(n / 4) rows-of-4
  UnstageJob job[IMAXJ];
};

__global__ __launch_bounds__(NTHREADS) void inv_copy_out(UnstageArgs a) {
  int j = 0;
  while (j + 1 < a.njobs && (int)blockIdx.x >= a.begin[j + 1]) ++j;
  const UnstageJob& U = a.job[j];
  const int r0 = ((int)blockIdx.x - a.begin[j]) * 4;
  if (r0 == 0 && threadIdx.x == 0 && U.idst) *U.idst = *U.isrc;
  for (int r = r0; r < r0 + 4 && r < U.n; ++r)
    for (int c = threadIdx.x; c < U.n; c += NTHREADS) U.dst[(int64_t)r * U.ldo + c] = U.src[(int64_t)r * U.n + c];
}

static bool graph_enabled() { return knobs().inv_graph != 0; }

// A cached chain is keyed by its SHAPE (stream, step count, per-job sizes / kinds,
// launch knobs): a call whose arguments differ only in values -- damping (scale,
// shift), factor / output / workspace pointers -- updates the instantiated graph's
// kernel nodes in place (hipGraphExecKernelNodeSetParams: launches already queued
// keep the arguments they were queued with) instead of building a new graph, so a
// damping schedule or a grid over (add, multiply) replays one graph.  An evicted
// entry waits for its last replay (an event recorded after it) before its graph is
// destroyed.
struct GraphEntry {
  hipStream_t stream = nullptr;
  int tmax = 0;
  int njobs = 0, tpw = 0;
  int n[IMAXJ] = {}, kind[IMAXJ] = {};
  InvArgs args{};    // phase-1 arguments the nodes hold now (step / begin cleared)
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipEvent_t last = nullptr;  // recorded after the latest replay
  std::vector<hipGraphNode_t> nodes;
  std::vector<int> node_step;
  unsigned long long used = 0;
};
static std::mutex g_graph_mu;
static GraphEntry g_graphs[8];
static unsigned long long g_graph_tick = 0;

static bool same_shape(const GraphEntry& e, const InvArgs& a, int Tmax, hipStream_t s) {
  if (!e.exec || e.stream != s || e.tmax != Tmax || e.njobs != a.njobs || e.tpw != a.tpw)
    return false;
  for (int j = 0; j < a.njobs; ++j)
    if (e.n[j] != a.job[j].n || e.kind[j] != a.job[j].kind) return false;
  return true;
}

static hipKernelNodeParams step_node(InvArgs& a, void** params, int total) {
  hipKernelNodeParams p{};
  params[0] = &a;
  p.func = reinterpret_cast<void*>(inv_step);
  p.gridDim = dim3(total);
  p.blockDim = dim3(NTHREADS);
  p.sharedMemBytes = 0;
  p.kernelParams = params;
  p.extra = nullptr;
  return p;
}

static void drop_entry(GraphEntry& e) {
  if (e.last) {
    (void)hipEventSynchronize(e.last);  // its last replay has finished
    (void)hipEventDestroy(e.last);
  }
  if (e.exec) (void)hipGraphExecDestroy(e.exec);
  if (e.graph) (void)hipGraphDestroy(e.graph);
  e = GraphEntry{};
}

// every cached graph: wait for its last replay, then destroy it (kfac_release)
void release_graphs() {
  std::lock_guard<std::mutex> lk(g_graph_mu);
  for (GraphEntry& e : g_graphs) drop_entry(e);
}

// steps 0 .. Tmax-1 as a replay of a cached graph
static int launch_steps_graph(const InvArgs& args, int Tmax, hipStream_t s) {
  InvArgs key;
  memcpy(&key, &args, sizeof(InvArgs));
  key.step = 0;
  for (int j = 0; j <= IMAXJ; ++j) key.begin[j] = 0;
  std::lock_guard<std::mutex> lk(g_graph_mu);
  GraphEntry* hit = nullptr;
  GraphEntry* lru = nullptr;
  for (GraphEntry& e : g_graphs) {
    if (same_shape(e, args, Tmax, s)) {
      // new values go into the nodes only once the entry's last replay has finished:
      // HIP gives no guarantee that a replay still queued keeps the arguments it was
      // launched with, so a busy entry is left alone (another one is used or built)
      if (memcmp(&e.args, &key, sizeof(InvArgs)) == 0 || hipEventQuery(e.last) == hipSuccess) {
        hit = &e;
        break;
      }
      continue;
    }
    if (!lru || e.used < lru->used) lru = &e;
  }
  if (!hit && !lru) {  // every entry is a busy one of this shape: the oldest, once idle
    lru = &g_graphs[0];
    for (GraphEntry& e : g_graphs)
      if (e.used < lru->used) lru = &e;
  }
  if (hit && memcmp(&hit->args, &key, sizeof(InvArgs)) != 0) {
    // same shape, other values: new arguments into the existing nodes
    for (size_t q = 0; q < hit->nodes.size(); ++q) {
      InvArgs a = args;
      const int total = step_args(a, hit->node_step[q]);
      void* params[1];
      hipKernelNodeParams p = step_node(a, params, total);
      if (hipGraphExecKernelNodeSetParams(hit->exec, hit->nodes[q], &p) != hipSuccess) {
        drop_entry(*hit);
        hit = nullptr;
        break;
      }
    }
    if (hit) hit->args = key;
  }
  if (!hit) {
    GraphEntry& e = *lru;
    drop_entry(e);
    if (hipGraphCreate(&e.graph, 0) != hipSuccess) return KFAC_ELAUNCH;
    hipGraphNode_t prev = nullptr;
    for (int k = 0; k < Tmax; ++k) {
      InvArgs a = args;
      const int total = step_args(a, k);
      if (total == 0) continue;
      void* params[1];
      hipKernelNodeParams p = step_node(a, params, total);
      hipGraphNode_t node;
      if (hipGraphAddKernelNode(&node, e.graph, prev ? &prev : nullptr, prev ? 1 : 0, &p) != hipSuccess) {
        drop_entry(e);
        return KFAC_ELAUNCH;
      }
      e.nodes.push_back(node);
      e.node_step.push_back(k);
      prev = node;
    }
    if (hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0) != hipSuccess ||
        hipEventCreateWithFlags(&e.last, hipEventDisableTiming) != hipSuccess) {
      drop_entry(e);
      return KFAC_ELAUNCH;
    }
    e.stream = s;
    e.tmax = Tmax;
    e.njobs = args.njobs;
    e.tpw = args.tpw;
    for (int j = 0; j < args.njobs; ++j) {
      e.n[j] = args.job[j].n;
      e.kind[j] = args.job[j].kind;
    }
    e.args = key;
    hit = &e;
  }
  hit->used = ++g_graph_tick;
  if (hipGraphLaunch(hit->exec, s) != hipSuccess) return KFAC_ELAUNCH;
  return hipEventRecord(hit->last, s) == hipSuccess ? KFAC_OK : KFAC_ELAUNCH;
}

// Phase 0 = the launch that reads F (step -1: builds R', zeroes info, factors tile
// (0,0)); phase 1 = steps 0 .. Tmax-1 and the outputs.
int invert_group(const kfac_invert_job* jobs, int njobs, char* ws, int32_t* info, hipStream_t s,
                 int phase) {
  InvArgs args;
  float* stage[IMAXJ];
  const int Tmax = fill_args(args, jobs, njobs, ws, info, stage);
  // 2 tasks per workgroup: +1.2 % on the MLP bench (3 A/B pairs), the early steps of a
  // 785 factor fit one round
  args.tpw = 2;
  bool all_fused = true;
  for (int i = 0; i < njobs; ++i) {
    args.job[i].xw = 1;
    args.job[i].fout = args.job[i].kind == KFAC_OUT_INV_CHOL;
    all_fused &= args.job[i].fout != 0;
  }
  // every L written by the steps: the steps replay a cached graph, outputs staged
  if (all_fused && graph_enabled()) {
    UnstageArgs ua{};
    ua.njobs = njobs;
    int blocks = 0;
    for (int i = 0; i < njobs; ++i) {
      InvJobDev& d = args.job[i];
      int* stage_info = reinterpret_cast<int*>(stage[i]) + (size_t)d.n * d.n;
      ua.job[i] = UnstageJob{stage[i], d.out, d.ldo, stage_info, d.info, d.n};
      ua.begin[i] = blocks;
      blocks += (d.n + 3) / 4;
      d.out = stage[i];
      d.ldo = d.n;
      d.info = stage_info;
    }
    ua.begin[njobs] = blocks;
    if (!phase) return launch_step(args, -1, s);
    const int rc = launch_steps_graph(args, Tmax, s);
    if (rc) return rc;
    hipLaunchKernelGGL(inv_copy_out, dim3(blocks), dim3(NTHREADS), 0, s, ua);
    KFAC_CHECK_LAUNCH();
    return KFAC_OK;
  }
  if (!phase) return launch_step(args, -1, s);
  for (int k = 0; k < Tmax; ++k) {
    const int rc = launch_step(args, k, s);
    if (rc) return rc;
  }
  return launch_outputs(args, s);
}

}  // namespace t32
}  // namespace kfac
