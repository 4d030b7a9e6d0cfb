// Tile-size generic part of the fp64 inversion: included by invert_merged.hip (NB = 32)
// and invert_blocked.hip (NB = 64) inside namespace kfac::t32 / kfac::t64, after NB.
// Device: tile access, MFMA tile products, the diagonal factorisation, the build of R',
// the output blocks, and the two kernels both paths launch (inv_xtx, inv_out).
// Host: workspace layout, InvArgs of a group, the grouped launch.
constexpr int DP = NB + 4;  // LDS pitch (doubles): conflict-free 16-byte MFMA operand reads (mfma_block)
constexpr int NBB = NB / 16;           // 16x16 MFMA blocks per tile edge
constexpr int BPW = NBB * NBB / 4;     // blocks of a tile product per wave (4 or 1)
constexpr int RSTEP = NTHREADS / NB;   // tile rows covered by one pass of the workgroup
static_assert(NB == 32 || NB == 64, "tile edge");

typedef double doublex4 __attribute__((ext_vector_type(4)));

struct InvJobDev {
  const float* F;
  int64_t ldF;
  float* out;
  int64_t ldo;
  double* W;   // Np x Np: R', then C below the diagonal (lower tiles)
  double* X;   // Np x Np: Z accumulators, then C^{-1} (lower tiles)
  double* Tm;  // Np x Np: scratch (X^T X)
  int* info;
  double scale, shift;
  int n, T, Np, kind;
  int xw;      // final strictly-lower X tiles in W (merged path) instead of X
  int fout;    // merged path, inverse-Cholesky output: the steps write L (no inv_out)
};

struct InvArgs {
  int njobs;
  int step;
  int tpw;         // inv_step: tasks per workgroup (1, or 2: see inv_step)
  int kend;        // blocked path: end of the panel block [step, kend)
  int ksplit;      // inv_bulk parts 1 / 2: end of the NEXT panel block [kend, ksplit)
  int part;        // inv_bulk: 0 every tile, 1 the next block's, 2 the rest (look-ahead)
  int begin[IMAXJ + 1];
  InvJobDev job[IMAXJ];
};

__device__ __forceinline__ int find_job(const InvArgs& a, int task) {
  int j = 0;
  while (j + 1 < a.njobs && task >= a.begin[j + 1]) ++j;
  return j;
}

__device__ __forceinline__ double* tile_ptr(double* base, int Np, int ti, int tj) {
  return base + ((int64_t)ti * NB) * Np + (int64_t)tj * NB;
}

// Up to three W / X workspace tiles into LDS with every load in flight together (one
// memory round trip instead of one per tile, and all of a thread's loads issued before
// its first LDS write); null destinations are skipped.  Plain accesses (tiles cross
// kernel boundaries only): 16-byte loads and LDS stores, two doubles per lane.
__device__ __forceinline__ void load_tiles(double* l0, const double* g0, double* l1, const double* g1,
                                           double* l2, const double* g2, int Np) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  constexpr int LPR = NB / 2;                  // lanes per tile row
  constexpr int RS2 = NTHREADS / LPR;          // rows per pass
  constexpr int PER2 = NB * NB / (2 * NTHREADS);
  const int c = 2 * (threadIdx.x % LPR), r0 = threadIdx.x / LPR;
  d2 v0[PER2], v1[PER2], v2[PER2];
#pragma unroll
  for (int q = 0; q < PER2; ++q) {
    const int64_t off = (int64_t)(r0 + RS2 * q) * Np + c;
    v0[q] = *reinterpret_cast<const d2*>(g0 + off);
    if (l1) v1[q] = *reinterpret_cast<const d2*>(g1 + off);
    if (l2) v2[q] = *reinterpret_cast<const d2*>(g2 + off);
  }
#pragma unroll
  for (int q = 0; q < PER2; ++q) {
    const int o = (r0 + RS2 * q) * DP + c;
    *reinterpret_cast<d2*>(l0 + o) = v0[q];
    if (l1) *reinterpret_cast<d2*>(l1 + o) = v1[q];
    if (l2) *reinterpret_cast<d2*>(l2 + o) = v2[q];
  }
}

__device__ __forceinline__ void load_tile(double* lds, const double* g, int Np) {
  load_tiles(lds, g, nullptr, nullptr, nullptr, nullptr, Np);
}

__device__ __forceinline__ void store_tile(double* g, const double* lds, int Np) {
  for (int e = threadIdx.x; e < NB * NB; e += NTHREADS) {
    const int r = e / NB, c = e % NB;
    g[(int64_t)r * Np + c] = lds[r * DP + c];
  }
}

// ---------------------------------------------------------------- MFMA f64 blocks
// One wave accumulates a 16x16 block: acc += A(16xK) * op(B), A rows at `a` (pitch
// lda), B either (K x 16) at `b` (trans=false) or (16 x K) at `b` read as B^T.
// v_mfma_f64_16x16x4_f64: lane l holds A[l&15][k0 + (l>>4)], B[k0 + (l>>4)][l&15];
// result register v of lane l is C[(l>>4) + 4v][l&15].
// acc += A[16 x K] * B (TRANS_B: B[16 x K] read as rows, i.e. A B^T; else B[K x 16]).
// Each lane reads two consecutive k of its A row (and of its B row when TRANS_B) with
// ONE ds_read_b128 for two MFMAs: the first MFMA takes k0 + 2 kk, the second
// k0 + 2 kk + 1 (kk = lane >> 4), which covers k0 .. k0 + 7 -- the sum does not care
// which k a lane slot carries as long as A and B agree.  At the NB + 4 pitch the
// 16-byte reads are conflict-free; the compiler had paired two 8-byte reads into
// ds_read2_b64 (8 LDS cycles, 5 conflict cycles per instruction, profiles/r05y/).
template <bool TRANS_B>
__device__ __forceinline__ void mfma_block(const double* a, int lda, const double* b, int ldb, int K,
                                           doublex4& acc) {
  typedef double double2v __attribute__((ext_vector_type(2)));
  const int lane = threadIdx.x & 63;
  const int i = lane & 15, kk = lane >> 4;
  for (int k0 = 0; k0 < K; k0 += 8) {
    const double2v av = *reinterpret_cast<const double2v*>(a + i * lda + k0 + 2 * kk);
    double bv0, bv1;
    if (TRANS_B) {
      const double2v bv = *reinterpret_cast<const double2v*>(b + i * ldb + k0 + 2 * kk);
      bv0 = bv.x;
      bv1 = bv.y;
    } else {
      bv0 = b[(k0 + 2 * kk) * ldb + i];
      bv1 = b[(k0 + 2 * kk + 1) * ldb + i];
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv1, acc, 0, 0, 0);
  }
}

__device__ __forceinline__ int acc_row64(int v) { return ((threadIdx.x & 63) >> 4) + 4 * v; }

// 16x16 block x of wave w's share of a tile product: (block row, block column)
__device__ __forceinline__ int blk_r(int x) { return ((threadIdx.x >> 6) * BPW + x) / NBB; }
__device__ __forceinline__ int blk_c(int x) { return ((threadIdx.x >> 6) * BPW + x) % NBB; }

// Full NB x NB tile product into registers: wave w owns blocks w*BPW .. w*BPW+BPW-1
// (NB = 64: block row w; NB = 32: one block), acc[x] = block (blk_r(x), blk_c(x)).
template <bool TRANS_B>
__device__ __forceinline__ void gemm64(const double* A, const double* B, doublex4 (&acc)[BPW]) {
#pragma unroll
  for (int x = 0; x < BPW; ++x) {
    acc[x] = doublex4{0.0, 0.0, 0.0, 0.0};
    if (TRANS_B)
      mfma_block<true>(A + 16 * blk_r(x) * DP, DP, B + 16 * blk_c(x) * DP, DP, NB, acc[x]);
    else
      mfma_block<false>(A + 16 * blk_r(x) * DP, DP, B + 16 * blk_c(x), DP, NB, acc[x]);
  }
}

// global[tile](r, c) = alpha * acc (+ global if accumulate)   (acc from gemm64)
__device__ __forceinline__ void store_acc_global(double* g, int Np, const doublex4 (&acc)[BPW],
                                                 double alpha, bool accumulate) {
  const int col = threadIdx.x & 15;
  auto at = [&](int x, int v) {
    return g + (int64_t)(16 * blk_r(x) + acc_row64(v)) * Np + 16 * blk_c(x) + col;
  };
  // every old value loaded before the first store
  double old[BPW][4];
#pragma unroll
  for (int x = 0; x < BPW; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) old[x][v] = accumulate ? *at(x, v) : 0.0;
#pragma unroll
  for (int x = 0; x < BPW; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double* p = at(x, v);
      *p = old[x][v] + alpha * acc[x][v];
    }
}

// acc (gemm64 layout) -> LDS tile
__device__ __forceinline__ void store_acc_lds(double* S, const doublex4 (&acc)[BPW]) {
  const int col = threadIdx.x & 15;
#pragma unroll
  for (int x = 0; x < BPW; ++x)
#pragma unroll
    for (int v = 0; v < 4; ++v) S[(16 * blk_r(x) + acc_row64(v)) * DP + 16 * blk_c(x) + col] = acc[x][v];
}

// 1/d: v_rcp_f64 + two Newton steps (~1 ulp) instead of the IEEE division sequence,
// which sits on the elimination's serial chain.
__device__ __forceinline__ double fast_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  return __builtin_fma(r, e, r);
}

// ------------------------------------------------ cross-lane helpers
// (a register-only elimination on DPP row_newbcast / permlane swaps and a 4-column LDS
// exchange were measured slower than the LDS broadcast below and removed: DESIGN.md §3.3)
__device__ __forceinline__ unsigned lo32(double x) { return (unsigned)__builtin_bit_cast(unsigned long long, x); }
__device__ __forceinline__ unsigned hi32(double x) { return (unsigned)(__builtin_bit_cast(unsigned long long, x) >> 32); }
__device__ __forceinline__ double mk64(unsigned lo, unsigned hi) {
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double lane_value_rt(double x, int lane) {  // lane: a constant
  return mk64((unsigned)__builtin_amdgcn_readlane((int)lo32(x), lane),
              (unsigned)__builtin_amdgcn_readlane((int)hi32(x), lane));
}

// --------------------------------------------------------- diagonal factorisation
// S (NB x NB lower, LDS) -> Y = chol(S)^{-1} (lower, LDS); S is destroyed.
// Blocked by 16: wave 0 eliminates each 16x16 diagonal block [D | I] -> I_k =
// D^{-1/2} L_unit^{-1}; the panel (C = S I_k^T, X_k = I_k Z_k) and the trailing /
// Z updates are 16x16 MFMA blocks spread over the 4 waves.  dg (>= NB+352 doubles)
// receives the pivots; its tail is scratch.
__device__ __forceinline__ void diag_factor(double* S, double* Y, double* dg) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // Y's off-diagonal 16-blocks start at zero (the Z blocks accumulate into them, the
  // upper ones stay zero); waves 1-3 clear them while wave 0 eliminates the first
  // diagonal block (each diagonal block is written whole by its own elimination, and
  // nothing reads an off-diagonal block before the barrier that ends the first panel)
  if (wave > 0) {
    typedef double dbl2 __attribute__((ext_vector_type(2)));
    const dbl2 z = {0.0, 0.0};
    // the (NBB - 1) NBB off-diagonal blocks in row order, 16 x 8 pairs of doubles each
    // (row pitch DP: 16-byte aligned rows)
    for (int e = tid - 64; e < (NBB - 1) * NBB * 128; e += NTHREADS - 64) {
      const int b = e >> 7, w = e & 127;
      const int bi = b / (NBB - 1), bo = b - bi * (NBB - 1), bj = bo + (bo >= bi);
      *reinterpret_cast<dbl2*>(&Y[(16 * bi + (w >> 3)) * DP + 16 * bj + 2 * (w & 7)]) = z;
    }
  }
  for (int kb = 0; kb < NBB; ++kb) {
    const int o = 16 * kb;
    // (1) one wave: unit-lower elimination of the 16x16 diagonal block [D | I] -> I_k.
    // Lane (r, g) keeps D[r][4g..4g+3] and Y[r][4g..4g+3] in registers; per column
    // the owners publish column j of D and row j of Y to LDS (`bc`, `by`), and every
    // lane reads what it needs in one batch (LDS ops of one wave complete in order,
    // so no barrier), then updates without per-entry selects (no divergent branches).
    if (wave == 0) {
      double* Sb = S + o * DP + o;
      double* Yb = Y + o * DP + o;
      double* bc = dg + NB;       // column j of D: 16 slots + 64 dummy slots
      double* by = dg + NB + 80;  // row j of Y: 16 slots + 4*64 dummy slots
      const int r = lane & 15, g = lane >> 4;
      double sv[4], yv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sv[q] = Sb[r * DP + 4 * g + q];
        yv[q] = (r == 4 * g + q) ? 1.0 : 0.0;
      }
      double piv = 1.0;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        // every lane writes (non-owners into private dummy slots): no divergent branches.
        // Column j is published with zeros above the diagonal, so the update below
        // needs no per-entry selects: entries left of column j take l * 0, and row j
        // of Y is exactly zero right of the diagonal (lower triangular by induction),
        // so a lane's Y entries right of column j take l * 0 too; rows r <= j take
        // l = 0.  (rr: r re-read each column so the compares stay in the loop body
        // instead of 64 hoisted lane masks spilling SGPRs.)
        int rr = r;
        asm volatile("" : "+v"(rr));
        bc[(g == (j >> 2)) ? rr : 16 + lane] = (rr >= j) ? sv[j & 3] : 0.0;
        double* yw = by + ((rr == j) ? 4 * g : 16 + 4 * lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) yw[q] = yv[q];
        // the pivot D[j][j] straight from its lane (j, j / 4) by readlane, so its
        // reciprocal (v_rcp_f64 + two Newton steps, ~1 ulp, instead of the IEEE
        // division's 11-op chain) runs while the LDS round trip is in flight
        const double d = lane_value_rt(sv[j & 3], j + 16 * (j >> 2));
        const double srj = bc[rr];
        double sc[4], yj[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          sc[q] = bc[4 * g + q];
          yj[q] = by[4 * g + q];
        }
        piv = (rr == j) ? d : piv;
        const double l = (rr > j) ? srj * fast_rcp(d) : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          sv[q] = __builtin_fma(-l, sc[q], sv[q]);
          yv[q] = __builtin_fma(-l, yj[q], yv[q]);
        }
      }
      if (g == 0) dg[o + r] = piv;
      const double rs = 1.0 / sqrt(piv);
#pragma unroll
      for (int q = 0; q < 4; ++q) Yb[r * DP + 4 * g + q] = (4 * g + q <= r) ? yv[q] * rs : 0.0;
    }
    // 32-tiles (NBB = 2): the one panel block is wave 0's, as the elimination, so its
    // reads of I and the in-place store below need no barrier (a wave's LDS operations
    // complete in order); 64-tiles spread the panel over waves 0-2
    if constexpr (NBB > 2) __syncthreads();
    // (2) panel: blocks ib > kb: C = S[ib][kb] I^T ;  blocks jb < kb: X = I Z[kb][jb]
    const int nC = NBB - 1 - kb, nX = kb;
    doublex4 acc = {0.0, 0.0, 0.0, 0.0};
    int mine = -1;
    if (wave < nC + nX) {  // nC + nX = NBB - 1 <= 3: at most one block per wave
      mine = wave;
      if (wave < nC) {
        const int ib = kb + 1 + wave;
        mfma_block<true>(S + 16 * ib * DP + o, DP, Y + o * DP + o, DP, 16, acc);
      } else {
        const int jb = wave - nC;
        mfma_block<false>(Y + o * DP + o, DP, Y + o * DP + 16 * jb, DP, 16, acc);
      }
    }
    if constexpr (NBB > 2) __syncthreads();
    if (mine >= 0) {
      const int col = lane & 15;
      double* dst = (mine < nC) ? S + 16 * (kb + 1 + mine) * DP + o : Y + o * DP + 16 * (mine - nC);
#pragma unroll
      for (int v = 0; v < 4; ++v) dst[acc_row64(v) * DP + col] = acc[v];
    }
    __syncthreads();
    if (kb == NBB - 1) break;
    // (3) trailing: S[ib][jb] -= C[ib] C[jb]^T (kb < jb <= ib); Z[ib][jb] -= C[ib] X[kb][jb] (jb <= kb)
    const int nT = (NBB - 1 - kb) * (NBB - kb) / 2, nZ = (NBB - 1 - kb) * (kb + 1);
    for (int t = wave; t < nT + nZ; t += 4) {
      doublex4 a2 = {0.0, 0.0, 0.0, 0.0};
      double* dst;
      if (t < nT) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= t) ++i;
        const int ib = kb + 1 + i, jb = kb + 1 + (t - i * (i + 1) / 2);
        mfma_block<true>(S + 16 * ib * DP + o, DP, S + 16 * jb * DP + o, DP, 16, a2);
        dst = S + 16 * ib * DP + 16 * jb;
      } else {
        const int u = t - nT;
        const int ib = kb + 1 + u / (kb + 1), jb = u % (kb + 1);
        mfma_block<false>(S + 16 * ib * DP + o, DP, Y + o * DP + 16 * jb, DP, 16, a2);
        dst = Y + 16 * ib * DP + 16 * jb;
      }
      const int col = lane & 15;
#pragma unroll
      for (int v = 0; v < 4; ++v) dst[acc_row64(v) * DP + col] -= a2[v];
    }
    __syncthreads();
  }
}

// Pivot check of the factored diagonal tile d: info = first global column whose
// pivot is not positive (+1), one ballot of wave 0 (no serial scan).
__device__ __forceinline__ void check_pivots(const InvJobDev& J, int d, const double* dg) {
  if (!J.info || threadIdx.x >= 64) return;
  const int c = threadIdx.x, g = d * NB + c;
  const unsigned long long bad = __ballot(c < NB && g < J.n && !(dg[c] > 0.0));
  if (bad && c == 0) atomicCAS(J.info, 0, d * NB + __ffsll(bad));
}

// ------------------------------------------------------------------- build R'
// R'[i][c] = scale*(F[fi][fc] + F[fc][fi])/2 + shift*[i==c], fi = n-1-i, fc = n-1-c.
// Both source blocks are read row-coalesced into LDS (fp32, P and Q: NB x (NB+1) floats
// each), then combined; tile (ti, tj) goes to W (and a copy to LDS `copy` when
// non-null: the merged build's task 0 factors tile (0,0) straight from it).
__device__ __forceinline__ void build_tile(const InvJobDev& J, int ti, int tj, float* P, float* Q,
                                           double* copy) {
  const int n = J.n, i0 = ti * NB, c0 = tj * NB;
  constexpr int PER = NB * NB / NTHREADS;
  const int cc = threadIdx.x % NB, r0 = threadIdx.x / NB;
  float pv[PER], qv[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int a = r0 + RSTEP * q;
    // row fi = n-1-(i0+a), column fc = n-1-(c0+cc): consecutive lanes -> consecutive fc (descending)
    const int i = i0 + a, c = c0 + cc;
    pv[q] = (i < n && c < n) ? J.F[(int64_t)(n - 1 - i) * J.ldF + (n - 1 - c)] : 0.f;
    const int ib = i0 + cc, cb = c0 + a;  // Q[a][cc] = F[n-1-(c0+a)][n-1-(i0+cc)]
    qv[q] = (ib < n && cb < n) ? J.F[(int64_t)(n - 1 - cb) * J.ldF + (n - 1 - ib)] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    P[(r0 + RSTEP * q) * (NB + 1) + cc] = pv[q];
    Q[(r0 + RSTEP * q) * (NB + 1) + cc] = qv[q];
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int a = r0 + RSTEP * q, i = i0 + a, c = c0 + cc;
    double v;
    if (i < n && c < n) {
      const double sym = 0.5 * ((double)P[a * (NB + 1) + cc] + (double)Q[cc * (NB + 1) + a]);
      v = J.scale * sym + (i == c ? J.shift : 0.0);
    } else {
      v = (i == c) ? 1.0 : 0.0;  // identity padding keeps the padded block trivial
    }
    J.W[(int64_t)i * J.Np + c] = v;
    if (copy) copy[a * DP + cc] = v;
    if (ti != tj) J.X[(int64_t)i * J.Np + c] = 0.0;  // Z accumulators start at 0
  }
}

// Output block of the final inverse tile X(a, b), a >= b, from LDS (pitch DP):
// L[n-1-q][n-1-r] = X[r][q] (r in tile a, q in tile b).  Output rows are walked
// with consecutive lanes on consecutive output columns (descending r): coalesced
// stores.  zero = true writes the (all-zero) block of the upper tile X(b, a) instead.
__device__ __forceinline__ void emit_out(const InvJobDev& J, int a, int b, const double* lds,
                                         bool zero = false) {
  const int n = J.n;
  for (int e = threadIdx.x; e < NB * NB; e += NTHREADS) {
    const int cl = e / NB, rl = NB - 1 - (e % NB);
    const int r = a * NB + rl, q = b * NB + cl;
    if (r >= n || q >= n) continue;
    J.out[(int64_t)(n - 1 - q) * J.ldo + (n - 1 - r)] = zero ? 0.f : (float)lds[rl * DP + cl];
  }
}

// Upper zero block of L for the strictly-lower tile (ti, tj): X(tj, ti) = 0, i.e.
// L[n-1-q][n-1-r] = 0 for r in tile tj, q in tile ti.
__device__ __forceinline__ void emit_zero_block(const InvJobDev& J, int ti, int tj) {
  const int n = J.n;
  for (int e = threadIdx.x; e < NB * NB; e += NTHREADS) {
    const int ql = e / NB, rl = NB - 1 - (e % NB);
    const int r = tj * NB + rl, q = ti * NB + ql;
    if (r >= n || q >= n) continue;
    J.out[(int64_t)(n - 1 - q) * J.ldo + (n - 1 - r)] = 0.f;
  }
}

// final inverse X tile (a >= b): the merged path leaves the strictly-lower tiles in W
// (xw, see inv_step), the blocked path everything in X
__device__ __forceinline__ const double* x_tile(const InvJobDev& J, int a, int b) {
  return tile_ptr(a > b && J.xw ? J.W : J.X, J.Np, a, b);
}

// Y[a][b] = sum_{m >= a} X[m][a]^T X[m][b]   (lower tiles, a >= b)
__global__ __launch_bounds__(NTHREADS) void inv_xtx(InvArgs args) {
  __shared__ __attribute__((aligned(16))) double A[NB * DP];
  __shared__ __attribute__((aligned(16))) double B[NB * DP];
  const int jb = find_job(args, blockIdx.x);
  const InvJobDev& J = args.job[jb];
  int a, b;
  tri_decode(blockIdx.x - args.begin[jb], a, b);
  const int lane = threadIdx.x & 63;
  doublex4 acc[BPW];
#pragma unroll
  for (int q = 0; q < BPW; ++q) acc[q] = doublex4{0.0, 0.0, 0.0, 0.0};
  for (int m = a; m < J.T; ++m) {
    load_tiles(A, x_tile(J, m, a), B, x_tile(J, m, b), nullptr, nullptr, J.Np);  // A read transposed
    __syncthreads();
    const int i = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int q = 0; q < BPW; ++q)
      for (int k0 = 0; k0 < NB; k0 += 4) {
        const double av = A[(k0 + kk) * DP + 16 * blk_r(q) + i];  // (X^T)[row][k] = X[k][row]
        const double bv = B[(k0 + kk) * DP + 16 * blk_c(q) + i];
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
      }
    __syncthreads();
  }
  store_acc_global(tile_ptr(J.Tm, J.Np, a, b), J.Np, acc, 1.0, false);
}

// ------------------------------------------------------------------- output
__global__ __launch_bounds__(NTHREADS) void inv_out(InvArgs args) {
  const int jb = find_job(args, blockIdx.x);
  const InvJobDev& J = args.job[jb];
  const int local = blockIdx.x - args.begin[jb];
  const int ti = local / J.T, tj = local - ti * J.T;
  const int n = J.n;
  for (int e = threadIdx.x; e < NB * NB; e += NTHREADS) {
    const int i = ti * NB + e / NB, c = tj * NB + e % NB;
    if (i >= n || c >= n) continue;
    double v;
    if (J.kind == KFAC_OUT_INV_CHOL) {
      const int r = n - 1 - c, q = n - 1 - i;  // L[i][c] = X[r][q], r >= q
      v = (i >= c) ? ((r / NB) > (q / NB) && J.xw ? J.W : J.X)[(int64_t)r * J.Np + q] : 0.0;
    } else {
      const int a = n - 1 - i, b = n - 1 - c;
      v = (a >= b) ? J.Tm[(int64_t)a * J.Np + b] : J.Tm[(int64_t)b * J.Np + a];
    }
    J.out[(int64_t)i * J.ldo + c] = (float)v;
  }
}

// ---------------------------------------------------------------- host side
// A job's workspace region: W, X, Tm (Np x Np doubles each), then the staging area of
// the graph-replayed merged chain: L (n x n fp32) and the verdict.
static size_t stage_bytes(int64_t n) { return align_up((size_t)(n * n) * sizeof(float) + 256, 256); }

size_t job_ws(const kfac_invert_job& j) {
  const int64_t T = cdiv(j.n, NB), Np = T * NB;
  return 3 * align_up((size_t)(Np * Np) * sizeof(double), 256) + stage_bytes(j.n);
}

// InvArgs of a group of jobs whose regions start at `ws`; returns the most tiles per
// edge.  tpw / xw / fout and the per-launch fields are the path's to set.  `stage`
// (may be null) receives each job's staging area.
static int fill_args(InvArgs& args, const kfac_invert_job* jobs, int njobs, char* ws, int32_t* info,
                     float** stage) {
  memset(&args, 0, sizeof(args));  // (padding too: the graph cache compares the bytes)
  args.njobs = njobs;
  int Tmax = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_invert_job& jb = jobs[i];
    InvJobDev& d = args.job[i];
    d.F = jb.F;
    d.ldF = jb.ldF;
    d.out = jb.out;
    d.ldo = jb.ldo;
    d.n = jb.n;
    d.T = (int)cdiv(jb.n, NB);
    d.Np = d.T * NB;
    d.kind = jb.out_kind;
    d.scale = jb.scale;
    d.shift = jb.shift;
    d.info = info ? info + i : nullptr;
    const size_t mat = align_up((size_t)d.Np * d.Np * sizeof(double), 256);
    d.W = reinterpret_cast<double*>(ws);
    d.X = reinterpret_cast<double*>(ws + mat);
    d.Tm = reinterpret_cast<double*>(ws + 2 * mat);
    if (stage) stage[i] = reinterpret_cast<float*>(ws + 3 * mat);
    ws += job_ws(jb);
    Tmax = std::max(Tmax, d.T);
  }
  return Tmax;
}

// one launch over every job's tasks (count(job) workgroups each; none: no launch)
template <typename Count>
static int launch(void (*kern)(InvArgs), InvArgs& args, Count count, hipStream_t s) {
  int total = 0;
  for (int j = 0; j < args.njobs; ++j) {
    args.begin[j] = total;
    total += count(args.job[j]);
  }
  args.begin[args.njobs] = total;
  if (total == 0) return KFAC_OK;
  hipLaunchKernelGGL(kern, dim3(total), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

// After the elimination: Y = X^T X for the full-inverse jobs, then the output pass of
// every job whose L the steps did not already write (fout).
static int launch_outputs(InvArgs& args, hipStream_t s) {
  const int rc = launch(inv_xtx, args,
                        [](const InvJobDev& d) { return d.kind == KFAC_OUT_INVERSE ? d.T * (d.T + 1) / 2 : 0; }, s);
  if (rc) return rc;
  return launch(inv_out, args, [](const InvJobDev& d) { return d.fout ? 0 : d.T * d.T; }, s);
}
