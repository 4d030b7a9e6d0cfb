// Monte-Carlo GLM predictive under the INF posterior: exact logit draws without weight samples
// (kfac_inf_draws, kfac_inf_draws_outer).  With c = sqrt(w) entrywise, Z (nA x nG) and eps (r)
// standard normal (kfac_hip.h: w, F, B),
//   x = c o Z - w o [ UA mat(F^T q) UG^T ] ,   q = F vec(UA^T (c o Z) UG) + B^-1 eps
// is N(0, P^-1) exactly, and it moves logit row r = b*nc + c' of the linearised network by
//   dF[s][r] = < M_r o c , Z_s > - < y_r , q_s > ,   y_r = F t_r  (kfac_inf_cov's y).
// Every GEMM is a task list of 64x64 contract_tile tiles; an output element is ONE k-ordered
// chain from 0.  Products that are operands are formed in panel loaders and never stored.
//   y      : inf_launch_proj on the rows (outer: h, t, y; dense: x, t, y), R x r
//   F g    : inf_launch_proj's dense route with rows := draws, J := Z, W := C:
//            G[s] = F vec(UA^T (C o Z_s) UG), ns x r
//   q      : kfac_inf_draws_q, Q = G + E Binv^T: the y-launch result plus ONE second k-ordered
//            chain over r (E Binv^T from 0), added once; q_s reads draw s only
//   first  : outer: kfac_inf_draws_outer_tile, one task per (draw, 64-column g-tile, 64-sample
//            tile): W[b][g] = sum_a abar_b[a] (C[a][g] Z_s[a][g]) by fp32 MFMA over K = nA, the
//            left operand the raw a with the implicit ones column (Panel<KFAC_SAMPLEROWS>), the
//            right one Panel<KFAC_WROWMAJOR>, which rounds C*Z to fp32 as it loads; the tile
//            goes to LDS and is contracted with the raw Delta's g-tile for every class, one fma
//            chain in g order, Delta read through its transpose Dt (kfac_inf_draws_dt).
//            dense: kfac_inf_draws_tile<true>, Z (C o J)^T over one JSEG-long segment of
//            K = nA*nG, the B operand Panel<KFAC_WCHANNEL> of the raw rows with w = C
//   second : kfac_inf_draws_tile<false>, Q Y^T over one JSEG-long segment of r
//   reduce : F[s][r] (+)= sum_jobs ( sum_parts first - sum_segments second ), fp64, parts in part
//            order, jobs in job order.  No atomics; the difference is never taken in fp32.
#include "covariance_inf.h"

namespace kfac {

constexpr int KFAC_WROWMAJOR = 24;  // (k = a, j = g) = C[a*ld + g] * Z[a*ld + g]
constexpr int IWP = TILE + 1;       // LDS pitch of the W tile
static_assert(TILE * IWP <= 4 * PANEL, "the W tile fits the staging buffer");

// Z_s (nA x nG row-major) scaled entrywise by C (the same layout)
__device__ __forceinline__ OpDev wrowmajor_op(const float* Z, const float* C, int nA, int nG) {
  OpDev d{};
  d.ptr = Z; d.layout = KFAC_WROWMAJOR; d.rows = nA; d.cols = nG; d.ld = nG; d.ones = -1;
  d.sB = aux_bits(C);
  return d;
}

// Panel<ROWMAJOR>'s thread map and 16-byte loads on both factors; the product is rounded to
// fp32 here, once, before it is staged.
template <>
struct Panel<KFAC_WROWMAJOR> {
  static constexpr int PITCH = TILE + 4;
  const float* base;
  const float* w;
  int64_t ld, kend;
  int col, c4, r0, cols;
  bool vec;
  __device__ __forceinline__ void init(const OpDev& op, const float* base_, int col0, int tid,
                                       int64_t k_end, int64_t) {
    base = base_; w = aux_ptr(op.sB); ld = op.ld; kend = k_end; cols = op.cols;
    c4 = (tid & 15) * 4; r0 = tid >> 4; col = col0 + c4;
    vec = (col + 3 < cols) && ((ld & 3) == 0) &&
          (((reinterpret_cast<uintptr_t>(base) | reinterpret_cast<uintptr_t>(w)) & 15) == 0);
  }
  __device__ __forceinline__ void load(int64_t k, float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int64_t row = k + r0 + 16 * m;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < kend) {
        const int64_t off = row * ld + col;
        if (vec) {
          const float4 z = *reinterpret_cast<const float4*>(base + off);
          const float4 c = *reinterpret_cast<const float4*>(w + off);
          x = make_float4(c.x * z.x, c.y * z.y, c.z * z.z, c.w * z.w);
        } else {
          float e[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) e[q] = col + q < cols ? w[off + q] * base[off + q] : 0.f;
          x = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      v[4 * m + 0] = x.x; v[4 * m + 1] = x.y; v[4 * m + 2] = x.z; v[4 * m + 3] = x.w;
    }
  }
  __device__ __forceinline__ void store(float* lds, const float (&v)[8]) const {
#pragma unroll
    for (int m = 0; m < 2; ++m)
      *reinterpret_cast<float4*>(lds + (r0 + 16 * m) * PITCH + c4) =
          make_float4(v[4 * m], v[4 * m + 1], v[4 * m + 2], v[4 * m + 3]);
  }
};

struct InfDrawJobDev {
  const float* a;     // outer route: nb x cols, stride lda
  const float* D;     //              R x nG, stride ldD
  float* Dt;          //              nG x R
  const float* J;     // dense route: R x nA*nG, stride ldJ
  const float* C;     // nA*nG
  const float* Z;     // draw s at Z + s*ldZ
  const float* E;     // draw s at E + s*ldE, r values
  const float* Binv;  // r x r, stride ldB
  const float* Y;     // R x r   (the rows' projection)
  const float* G;     // ns x r  (the draws' projection, F g)
  float* Q;           // ns x r
  float* part1;       // outer: [draw][g-tile][R]; dense: [segment][row tile][draw tile][64 x 64]
  float* part2;       // [segment][row tile][draw tile][64 draws x 64 rows]
  int64_t lda, ldD, ldJ, ldZ, ldE, ldB, K;  // K = nA*nG
  int cols, ones, nA, nG, tg, r, qn;
  int nseg1, nseg2;   // parts of the first term (outer: tg), segments of the second
  int begin1, begin2, t_begin, q_begin;
};

struct InfDrawArgs {
  int njobs, nc, accumulate;
  int R, nb, ns, bt, rt, st;  // rows, samples, draws; 64-tiles of the samples, rows, draws
  int64_t ldF;
  float* F;
  int end1[CMAXJ], end2[CMAXJ], t_end[CMAXJ], q_end[CMAXJ];
  InfDrawJobDev job[CMAXJ];
};
static_assert(sizeof(InfDrawArgs) <= 4096, "kernel argument block");

// Dt = D^T (rows ldD apart), 64x64 tiles through LDS: both sides run along the lanes.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_draws_dt(InfDrawArgs args) {
  __shared__ float tile[TILE * IWP];
  const int task = blockIdx.x;
  const InfDrawJobDev& C = args.job[cov_find_job(args.t_end, args.njobs, task)];
  const int local = task - C.t_begin;
  const int r0 = (local / C.tg) * TILE, g0 = (local % C.tg) * TILE;
  const int x = threadIdx.x & 63, y0 = threadIdx.x >> 6;
  for (int y = y0; y < TILE; y += 4) {
    const int r = r0 + y, g = g0 + x;
    if (r < args.R && g < C.nG) tile[y * IWP + x] = C.D[(int64_t)r * C.ldD + g];
  }
  __syncthreads();
  for (int y = y0; y < TILE; y += 4) {
    const int g = g0 + y, r = r0 + x;
    if (r < args.R && g < C.nG) C.Dt[(int64_t)g * args.R + r] = tile[x * IWP + y];
  }
}

// One 64 (draw) x 64 (j) tile of Q = G + E Binv^T: Q[s][j] = G[s][j] + sum_k E[s][k] Binv[j][k].
__global__ __launch_bounds__(NTHREADS) void kfac_inf_draws_q(InfDrawArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfDrawJobDev& C = args.job[cov_find_job(args.q_end, args.njobs, task)];
  const int local = task - C.q_begin;
  const int s0 = (local / C.qn) * TILE, j0 = (local % C.qn) * TILE;
  const OpDev e = channel_op(C.E, C.r, args.ns, C.ldE);
  const OpDev bi = channel_op(C.Binv, C.r, C.r, C.ldB);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_CHANNEL, KFAC_CHANNEL>(e, s0, bi, j0, 0, C.r, false, true, lds, acc);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = j0 + (wave & 1) * 32 + (lane & 31);
  if (j >= C.r) return;
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int s = s0 + (wave >> 1) * 32 + acc_row(v, lane);
    if (s < args.ns) C.Q[(int64_t)s * C.r + j] = C.G[(int64_t)s * C.r + j] + acc[v];
  }
}

// The hot kernel: one (draw, g-tile, sample tile).  W = abar_tile (C o Z_s)[:, g-tile] by MFMA,
// then part[r] = sum_g W[b(r)][g] Delta[r][g] for the tile's rows r = b*nc + c, every c.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_draws_outer_tile(InfDrawArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfDrawJobDev& C = args.job[cov_find_job(args.end1, args.njobs, task)];
  const int local = task - C.begin1;
  const int per = C.tg * args.bt;
  const int s = local / per, rem = local - s * per;
  const int gt = rem / args.bt, b0 = (rem - gt * args.bt) * TILE, g0 = gt * TILE;
  const OpDev a = samplerows_op(C.a, C.cols, C.ones, args.nb, C.lda);
  const OpDev z = wrowmajor_op(C.Z + (int64_t)s * C.ldZ, C.C, C.nA, C.nG);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  // W[b][g] = sum_a abar_b[a] (C[a][g] Z_s[a][g])
  contract_tile<KFAC_SAMPLEROWS, KFAC_WROWMAJOR>(a, b0, z, g0, 0, C.nA, false, true, lds, acc);
  // (contract_tile leaves through a barrier: lds is free)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* w = lds + (wave >> 1) * 32 * IWP + (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) w[acc_row(v, lane) * IWP] = acc[v];
  __syncthreads();
  const int nc = args.nc, R = args.R;
  const int nrows = min(TILE, args.nb - b0) * nc;
  const int gl = min(TILE, C.nG - g0);
  const int64_t r0 = (int64_t)b0 * nc;
  const float* dt = C.Dt + (int64_t)g0 * R + r0;
  float* part = C.part1 + ((int64_t)s * C.tg + gt) * R + r0;
  for (int p = tid; p < nrows; p += NTHREADS) {
    const float* wb = lds + (p / nc) * IWP;
    const float* dp = dt + p;
    float sum = 0.f;
#pragma unroll 8
    for (int g = 0; g < gl; ++g) sum = fmaf(wb[g], dp[(int64_t)g * R], sum);
    part[p] = sum;
  }
}

// Partial: 64 draws x 64 rows over one JSEG-long K segment (kfac_glm_draws_tile's body).
// FIRST: Z (C o J)^T over K = nA*nG, the weight folded into the rows' panel; else Q Y^T over r.
template <bool FIRST>
__global__ __launch_bounds__(NTHREADS) void kfac_inf_draws_tile(InfDrawArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfDrawJobDev& C = args.job[cov_find_job(FIRST ? args.end1 : args.end2, args.njobs, task)];
  const int local = task - (FIRST ? C.begin1 : C.begin2);
  const int per = args.rt * args.st;
  const int seg = local / per, tile = local - seg * per;
  const int tr = tile / args.st, ts = tile - tr * args.st;
  const int64_t K = FIRST ? C.K : (int64_t)C.r;
  const int64_t k0 = (int64_t)seg * JSEG, k1 = min(K, k0 + JSEG);
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  if (FIRST) {
    const OpDev z = channel_op(C.Z, K, args.ns, C.ldZ);
    const OpDev j = wchannel_op(C.J, K, C.ldJ, args.R, nullptr, C.C, C.nG, WGRAM_FLAT);
    contract_tile<KFAC_CHANNEL, KFAC_WCHANNEL>(z, ts * TILE, j, tr * TILE, k0, k1, false, true, lds, acc);
  } else {
    const OpDev q = channel_op(C.Q, K, args.ns, K);
    const OpDev y = channel_op(C.Y, K, args.R, K);
    contract_tile<KFAC_CHANNEL, KFAC_CHANNEL>(q, ts * TILE, y, tr * TILE, k0, k1, false, true, lds, acc);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* dst = (FIRST ? C.part1 : C.part2) + (int64_t)local * JTILE2 + (wave >> 1) * 32 * TILE +
               (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) dst[acc_row(v, lane) * TILE] = acc[v];
}

// F[s][r] (+)= sum_jobs ( first's parts in part order - second's segments in segment order ),
// the jobs in job order, fp64.  Grid: draws x 256-row blocks, the row blocks of a draw adjacent.
template <bool OUTER>
__global__ __launch_bounds__(NTHREADS) void kfac_inf_draws_reduce(InfDrawArgs args, int rblocks) {
  const int s = blockIdx.x / rblocks;
  const int r = (blockIdx.x - s * rblocks) * NTHREADS + threadIdx.x;
  if (r >= args.R) return;
  const int64_t per = (int64_t)args.rt * args.st;
  // the element's place in a segment's tile partials
  const int64_t te = ((int64_t)(r >> 6) * args.st + (s >> 6)) * JTILE2 + (s & 63) * TILE + (r & 63);
  double total = 0.0;
  for (int j = 0; j < args.njobs; ++j) {
    const InfDrawJobDev& C = args.job[j];
    double s1 = 0.0, s2 = 0.0;
    if (OUTER) {
      const float* p1 = C.part1 + (int64_t)s * C.tg * args.R + r;
      for (int i = 0; i < C.nseg1; ++i) s1 += (double)p1[(int64_t)i * args.R];
    } else {
      for (int i = 0; i < C.nseg1; ++i) s1 += (double)C.part1[(int64_t)i * per * JTILE2 + te];
    }
    for (int i = 0; i < C.nseg2; ++i) s2 += (double)C.part2[(int64_t)i * per * JTILE2 + te];
    total += s1 - s2;
  }
  float* f = args.F + (int64_t)s * args.ldF + r;
  *f = args.accumulate ? (float)((double)*f + total) : (float)total;
}

// ------------------------------------------------------------------ host
// R = nb*nc for 32-bit row indices, or 0
static int64_t inf_draw_rows(int64_t nb, int nc, int64_t ns) {
  const int64_t lim = ((int64_t)1 << 31) - TILE;
  if (nb <= 0 || nc <= 0 || ns <= 0 || ns >= lim || nb >= lim / nc) return 0;
  return nb * nc;
}

static inline int64_t draw_nA(const kfac_inf_cov_job& q) { return q.nA; }
static inline int64_t draw_nA(const kfac_inf_cov_outer_job& q) { return (int64_t)q.cols + (q.has_ones != 0); }
static inline bool draw_rows_ok(const kfac_inf_cov_job& q) { return inf_job_ok(q); }
static inline bool draw_rows_ok(const kfac_inf_cov_outer_job& q) { return inf_outer_job_ok(q); }
static inline bool draw_dims_ok(const kfac_inf_cov_job& q) { return q.nA > 0 && q.nG > 0 && q.ra > 0 && q.rg > 0; }
static inline bool draw_dims_ok(const kfac_inf_cov_outer_job& q) {
  return q.cols > 0 && q.nG > 0 && q.ra > 0 && q.rg > 0;
}

// The F g projection's job: the dense route with J := Z, W := C (rows := draws).
template <class JOB>
static kfac_inf_cov_job draw_zjob(const JOB& j) {
  kfac_inf_cov_job z{};
  z.J = j.Z; z.ldJ = j.ldZ;
  z.nA = (int32_t)draw_nA(j.rows); z.nG = j.rows.nG;
  z.UA = j.rows.UA; z.ldA = j.rows.ldA; z.ra = j.rows.ra;
  z.UG = j.rows.UG; z.ldG = j.rows.ldG; z.rg = j.rows.rg;
  z.W = j.C; z.ldW = (int64_t)z.nA * z.nG;
  z.F = j.rows.F; z.ldF = j.rows.ldF;
  return z;
}

static size_t draw_tiles_bytes(int64_t K, int64_t R, int64_t ns) {
  return align_up((size_t)(cdiv(K, JSEG) * cdiv(R, TILE) * cdiv(ns, TILE)) * JTILE2 * sizeof(float), 256);
}
static size_t draw_dt_bytes(int64_t nG, int64_t R) { return align_up((size_t)R * (size_t)nG * sizeof(float), 256); }
static size_t draw_outer_part_bytes(int64_t nG, int64_t R, int64_t ns) {
  return align_up((size_t)ns * (size_t)cdiv(nG, TILE) * (size_t)R * sizeof(float), 256);
}

template <bool OUTER, class JOB>
static size_t inf_draws_bytes(const JOB* jobs, int njobs, int64_t nb, int nc, int64_t ns) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ) return 0;
  const int64_t R = inf_draw_rows(nb, nc, ns);
  if (!R) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    if (!draw_dims_ok(jobs[i].rows)) return 0;
    const InfDims d = inf_dims(jobs[i].rows, nb, nc);
    const InfDims dz = inf_dims(draw_zjob(jobs[i]), ns, 1);
    const int64_t nA = draw_nA(jobs[i].rows), nG = jobs[i].rows.nG, r = d.ra * d.rg;
    total += inf_hx_bytes(d) + 2 * inf_ty_bytes(d, R) + inf_hx_bytes(dz) + 3 * inf_ty_bytes(dz, ns);
    total += OUTER ? draw_dt_bytes(nG, R) + draw_outer_part_bytes(nG, R, ns) : draw_tiles_bytes(nA * nG, R, ns);
    total += draw_tiles_bytes(r, R, ns);
  }
  return total;
}

template <bool OUTER, class JOB>
static int inf_draws_call(const JOB* jobs, int njobs, int64_t nb, int nc, int64_t ns, int accumulate, float* F,
                          int64_t ldF, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (!jobs || njobs <= 0 || njobs > CMAXJ || !F) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i) {
    const JOB& q = jobs[i];
    if (!draw_rows_ok(q.rows) || !q.C || !q.Binv || !q.Z || !q.E) return KFAC_EINVAL;
    const int64_t r = (int64_t)q.rows.ra * q.rows.rg;
    if (q.ldB < r || q.ldE < r || q.ldZ < draw_nA(q.rows) * q.rows.nG) return KFAC_EINVAL;
  }
  const int64_t R = inf_draw_rows(nb, nc, ns);
  if (!R || ldF < R) return KFAC_EINVAL;
  const int64_t lim = ((int64_t)1 << 31) - TILE;
  const bool have = workspace && workspace_bytes >= inf_draws_bytes<OUTER>(jobs, njobs, nb, nc, ns);
  InfArgs ap{}, az{};  // the projections of the rows (y) and of the draws (F g)
  InfDrawArgs args{};
  ap.njobs = az.njobs = args.njobs = njobs;
  ap.nc = args.nc = nc;
  ap.rows = (int)R;
  ap.nb = nb;
  az.nc = 1;
  az.rows = (int)ns;
  az.nb = ns;
  args.accumulate = accumulate;
  args.R = (int)R;
  args.nb = (int)nb;
  args.ns = (int)ns;
  args.bt = (int)cdiv(nb, TILE);
  args.rt = (int)cdiv(R, TILE);
  args.st = (int)cdiv(ns, TILE);
  args.ldF = ldF;
  args.F = F;
  const int64_t tiles = (int64_t)args.rt * args.st, rblocks = cdiv(R, NTHREADS);
  if (tiles >= lim || ns >= lim / rblocks) return KFAC_EINVAL;
  char* ws = have ? (char*)workspace : nullptr;
  int64_t np[3] = {0, 0, 0}, nz[3] = {0, 0, 0}, n1 = 0, n2 = 0, nt = 0, nq = 0;
  for (int i = 0; i < njobs; ++i) {
    const JOB& q = jobs[i];
    const kfac_inf_cov_job zj = draw_zjob(q);
    const InfDims d = inf_dims(q.rows, nb, nc), dz = inf_dims(zj, ns, 1);
    int64_t hcols, hm, hn;
    inf_set_operands(ap.job[i], q.rows);
    inf_h_shape(q.rows, nb, nc, hcols, hm, hn);
    if (!inf_fill_proj(ap, i, d, hcols, hm, hn, ws, np)) return KFAC_EINVAL;
    inf_set_operands(az.job[i], zj);
    inf_h_shape(zj, ns, 1, hcols, hm, hn);
    if (!inf_fill_proj(az, i, dz, hcols, hm, hn, ws, nz)) return KFAC_EINVAL;
    InfDrawJobDev& c = args.job[i];
    c.a = ap.job[i].a; c.D = ap.job[i].D; c.J = ap.job[i].J;
    c.lda = ap.job[i].lda; c.ldD = ap.job[i].ldD; c.ldJ = ap.job[i].ldJ;
    c.cols = ap.job[i].cols; c.ones = ap.job[i].ones;
    c.C = q.C; c.Z = q.Z; c.E = q.E; c.Binv = q.Binv;
    c.ldZ = q.ldZ; c.ldE = q.ldE; c.ldB = q.ldB;
    c.nA = (int)d.nA; c.nG = (int)d.nG; c.r = (int)(d.ra * d.rg);
    c.K = d.nA * d.nG;
    c.tg = (int)cdiv(d.nG, TILE);
    c.qn = (int)cdiv(c.r, TILE);
    if (cdiv(c.K, JSEG) >= lim) return KFAC_EINVAL;
    c.nseg1 = OUTER ? c.tg : (int)cdiv(c.K, JSEG);
    c.nseg2 = (int)cdiv(c.r, JSEG);
    c.begin1 = (int)n1; c.begin2 = (int)n2; c.t_begin = (int)nt; c.q_begin = (int)nq;
    const int64_t per = OUTER ? (int64_t)c.tg * args.bt : tiles;
    const int64_t count = OUTER ? ns : (int64_t)c.nseg1;
    if (per >= lim || count >= lim / per || c.nseg2 >= lim / tiles) return KFAC_EINVAL;
    n1 += count * per;
    n2 += c.nseg2 * tiles;
    nt += (int64_t)args.rt * c.tg;
    nq += (int64_t)args.st * c.qn;
    if (n1 >= lim || n2 >= lim || nt >= lim || nq >= lim) return KFAC_EINVAL;
    args.end1[i] = (int)n1; args.end2[i] = (int)n2; args.t_end[i] = (int)nt; args.q_end[i] = (int)nq;
    if (ws) {
      c.Y = ap.job[i].Y;
      c.G = az.job[i].Y;
      c.Q = reinterpret_cast<float*>(ws); ws += inf_ty_bytes(dz, ns);
      if (OUTER) {
        c.Dt = reinterpret_cast<float*>(ws); ws += draw_dt_bytes(d.nG, R);
        c.part1 = reinterpret_cast<float*>(ws); ws += draw_outer_part_bytes(d.nG, R, ns);
      } else {
        c.part1 = reinterpret_cast<float*>(ws); ws += draw_tiles_bytes(c.K, R, ns);
      }
      c.part2 = reinterpret_cast<float*>(ws); ws += draw_tiles_bytes(c.r, R, ns);
    }
  }
  if (!have) return KFAC_EWORKSPACE;
  int rc = inf_launch_proj(ap, OUTER, np, s);
  if (rc != KFAC_OK) return rc;
  rc = inf_launch_proj(az, false, nz, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_inf_draws_q, dim3((unsigned)nq), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  if (OUTER) {
    hipLaunchKernelGGL(kfac_inf_draws_dt, dim3((unsigned)nt), dim3(NTHREADS), 0, s, args);
    KFAC_CHECK_LAUNCH();
    hipLaunchKernelGGL(kfac_inf_draws_outer_tile, dim3((unsigned)n1), dim3(NTHREADS), 0, s, args);
  } else {
    hipLaunchKernelGGL(kfac_inf_draws_tile<true>, dim3((unsigned)n1), dim3(NTHREADS), 0, s, args);
  }
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_inf_draws_tile<false>, dim3((unsigned)n2), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kfac_inf_draws_reduce<OUTER>, dim3((unsigned)(ns * rblocks)), dim3(NTHREADS), 0, s, args,
                     (int)rblocks);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_inf_draws_workspace_bytes(const kfac_inf_draw_job* jobs, int njobs, int64_t nb, int nc,
                                                 int64_t ns) {
  return inf_draws_bytes<false>(jobs, njobs, nb, nc, ns);
}

extern "C" int kfac_inf_draws(const kfac_inf_draw_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                              int accumulate, float* F, int64_t ldF, void* workspace, size_t workspace_bytes,
                              kfac_stream_t stream) {
  return inf_draws_call<false>(jobs, njobs, nb, nc, ns, accumulate, F, ldF, workspace, workspace_bytes,
                               (hipStream_t)stream);
}

extern "C" size_t kfac_inf_draws_outer_workspace_bytes(const kfac_inf_draw_outer_job* jobs, int njobs, int64_t nb,
                                                       int nc, int64_t ns) {
  return inf_draws_bytes<true>(jobs, njobs, nb, nc, ns);
}

extern "C" int kfac_inf_draws_outer(const kfac_inf_draw_outer_job* jobs, int njobs, int64_t nb, int nc, int64_t ns,
                                    int accumulate, float* F, int64_t ldF, void* workspace,
                                    size_t workspace_bytes, kfac_stream_t stream) {
  return inf_draws_call<true>(jobs, njobs, nb, nc, ns, accumulate, F, ldF, workspace, workspace_bytes,
                              (hipStream_t)stream);
}
