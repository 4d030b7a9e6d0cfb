// GLM predictive under the INF posterior for any number of outputs (kfac_inf_cov_tiled,
// kfac_inf_cov_outer_tiled): covariance_inf.hip's mathematics with the CLASSES tiled.
//   cov[b][c][c'] (+)= sum_jobs [ sum_k w_b[k] R_b[c][k] R_b[c'][k] - < y_{b,c}, y_{b,c'} > ] ,  y = F t
//   dense  R_b = the raw rows J (stride ldJ), k over nA*nG, w = W flat
//   outer  R_b = Delta_b (stride ldD), k over nG, w_b = rho_b = row ra of sample b in HR
// The projections h | x, t, y are the capped calls' own launches (inf_launch_proj,
// covariance_inf.h), over all nb*nc rows at once.  A sample's block is then cut into 64x64
// class tiles, ntile = ceil(nc / 64), tile pairs ti >= tj, exactly as covariance_tiled.hip and
// covariance_wtiled.hip cut it:
//   gram    ONE launch for both terms, one task per (job, sample b, term, K segment, tile
//           pair).  Term 1 is covariance_wtiled.hip's weighted tile on the raw rows at their
//           own leading dimension: the A operand the plain CHANNEL panel of tile ti's rows, the
//           B operand Panel<KFAC_WCHANNEL>, tile tj's rows times the k-row's weight as they
//           are loaded.  Term 2 is covariance_tiled.hip's plain tile (cov_joint_gram_tile) on
//           Y_b (nc x r).  A diagonal tile skips its upper quadrant in both.  The 64x64 fp32
//           partials go to [b][pair][segment], one buffer per term.
//   reduce  per (sample, tile pair): sum_jobs (sum_seg part1 - sum_seg part2), segments in
//           segment order, jobs in job order, all in fp64: the two terms stay separate fp32
//           partials and their difference is formed in fp64.  The lower element is written
//           with its mirror into cov[b] (nc x nc contiguous); not clamped.  No atomics.
// K is cut into segments [s*JSEG, (s+1)*JSEG) by K alone (nA*nG or nG for term 1, r for term
// 2) and an element of a partial is one k-ordered fma chain from 0 over its segment.  Hence a
// block depends on its sample alone (chunking the samples changes no bit), two calls give
// identical bits, every block is bitwise symmetric, and with F = 0 the dense call gives the
// bits of kfac_kron_cov_full_tiled (nt = 1) on the same J and W with VA, VG identities: one
// tile body, one segmentation, one reduce order, and x * 1, s - 0 are exact.
// Tasks are ordered (job, sample, term 1's segments then term 2's, tile pair), so the tasks
// that share a sample's row panels are in flight together.
#include "covariance_inf.h"

namespace kfac {

struct InfTiledJobDev {
  const float* R;  // term 1: the raw rows, sample b at R + b*nc*ldR
  const float* w;  // term 1: sample b's weights at w + b*stride_b
  const float* Y;  // term 2: nb*nc x r, r contiguous per row
  float* part1;    // [sample][tile pair][segment][64 x 64]
  float* part2;
  int64_t K1, ldR, stride_b;
  int r, nseg1, nseg2, begin;  // begin: first task of this job
};

struct InfTiledArgs {
  int njobs, nc, accumulate, npairs;
  int64_t nb;
  float* cov;
  int end[CMAXJ];
  InfTiledJobDev x[CMAXJ];
};
static_assert(sizeof(InfTiledArgs) <= 4096, "kernel argument block");

// Gram partial: one tile pair of one sample of one job over one K segment of one term.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_tiled_gram(InfTiledArgs args) {
  __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
  const int task = blockIdx.x;
  const InfTiledJobDev& G = args.x[cov_find_job(args.end, args.njobs, task)];
  const int local = task - G.begin;
  const int q = local / args.npairs, pair = local - q * args.npairs;
  const int nseg = G.nseg1 + G.nseg2;
  const int64_t b = q / nseg;
  int seg = q - (int)b * nseg;
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int64_t tile = b * args.npairs + pair;
  if (seg >= G.nseg1) {
    seg -= G.nseg1;
    const int64_t k0 = (int64_t)seg * JSEG;
    cov_joint_gram_tile(G.Y + b * args.nc * G.r, G.r, args.nc, ti, tj, k0, min((int64_t)G.r, k0 + JSEG),
                        G.part2 + (tile * G.nseg2 + seg) * JTILE2, lds);
    return;
  }
  const int64_t k0 = (int64_t)seg * JSEG, k1 = min(G.K1, k0 + JSEG);
  const float* R = G.R + b * args.nc * G.ldR;
  const OpDev xa = channel_op(R, G.K1, args.nc, G.ldR);
  const OpDev xw = wchannel_op(R, G.K1, G.ldR, args.nc, nullptr, G.w + b * G.stride_b, 0, WGRAM_FLAT);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool active = !(ti == tj && wave == 1);  // quadrant (0, 1) of a diagonal tile
  floatx16 acc;
#pragma unroll
  for (int v = 0; v < 16; ++v) acc[v] = 0.f;
  contract_tile<KFAC_CHANNEL, KFAC_WCHANNEL>(xa, ti * TILE, xw, tj * TILE, k0, k1, false, active, lds, acc);
  if (!active) return;
  float* dst = G.part1 + (tile * G.nseg1 + seg) * JTILE2 + (wave >> 1) * 32 * TILE + (wave & 1) * 32 + (lane & 31);
#pragma unroll
  for (int v = 0; v < 16; ++v) dst[acc_row(v, lane) * TILE] = acc[v];
}

// cov[b] tile (ti >= tj) (+)= sum over jobs (in job order) of (term 1's segment sum - term
// 2's), each in segment order, fp64.  Grid (nb * tile pairs, JTILE2 / NTHREADS): a block owns
// four rows of the tile, a thread one element, as the tiled reduce.
__global__ __launch_bounds__(NTHREADS) void kfac_inf_tiled_reduce(InfTiledArgs args) {
  const int64_t b = blockIdx.x / args.npairs;
  const int pair = blockIdx.x - (int)b * args.npairs;
  int ti, tj;
  tri_decode(pair, ti, tj);
  const int nc = args.nc;
  const int e = blockIdx.y * NTHREADS + threadIdx.x;
  const int r = ti * TILE + (e >> 6), c = tj * TILE + (e & (TILE - 1));
  if (r >= nc || c > r) return;
  const int64_t tile = b * args.npairs + pair;
  double total = 0.0;
  for (int j = 0; j < args.njobs; ++j) {
    const InfTiledJobDev& G = args.x[j];
    const float* p1 = G.part1 + tile * G.nseg1 * JTILE2 + e;
    const float* p2 = G.part2 + tile * G.nseg2 * JTILE2 + e;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < G.nseg1; ++i) s1 += (double)p1[(int64_t)i * JTILE2];
    for (int i = 0; i < G.nseg2; ++i) s2 += (double)p2[(int64_t)i * JTILE2];
    total += s1 - s2;
  }
  float* cov = args.cov + b * nc * nc;
  float* lo = cov + (int64_t)r * nc + c;
  const float v = args.accumulate ? (float)((double)*lo + total) : (float)total;
  *lo = v;
  cov[(int64_t)c * nc + r] = v;
}

static bool inf_tiled_call_ok(const void* jobs, int njobs) { return jobs && njobs > 0 && njobs <= CMAXJ; }

static size_t inf_tiled_partial_bytes(int64_t nb, int nc, int64_t K) {
  return align_up((size_t)(nb * tiled_npairs(nc) * cdiv(K, JSEG)) * JTILE2 * sizeof(float), 256);
}
static size_t inf_tiled_job_bytes(const InfDims& d, int64_t nb, int nc) {
  return inf_hx_bytes(d) + 2 * inf_ty_bytes(d, nb * nc) + inf_tiled_partial_bytes(nb, nc, d.k1) +
         inf_tiled_partial_bytes(nb, nc, d.ra * d.rg);
}

template <class Job>
static size_t inf_tiled_bytes(const Job* jobs, int njobs, int64_t nb, int nc) {
  if (!inf_tiled_call_ok(jobs, njobs) || !tiled_rows(nb, nc)) return 0;
  size_t total = 0;
  for (int i = 0; i < njobs; ++i) {
    const InfDims d = inf_dims(jobs[i], nb, nc);
    if (d.nA <= 0 || d.nG <= 0 || d.ra <= 0 || d.rg <= 0) return 0;
    total += inf_tiled_job_bytes(d, nb, nc);
  }
  return total;
}

// job i of the Gram launch: nb samples x (term 1's + term 2's segments) x tile pairs; false:
// the tasks (and with them the reduce's nb * tile pairs blocks) do not fit 31 bits
static bool inf_tiled_add_job(InfTiledArgs& a, int i, int64_t K1, int64_t r, int64_t& ntasks) {
  const int64_t lim = (int64_t)1 << 31;
  InfTiledJobDev& g = a.x[i];
  const int64_t nseg1 = cdiv(K1, JSEG), nseg2 = cdiv(r, JSEG), nseg = nseg1 + nseg2;  // each < 2^52
  g.K1 = K1;
  g.r = (int)r;
  g.begin = (int)ntasks;
  if (nseg >= lim / a.npairs || a.nb >= lim / (nseg * a.npairs)) return false;
  g.nseg1 = (int)nseg1;
  g.nseg2 = (int)nseg2;
  ntasks += a.nb * nseg * a.npairs;
  if (ntasks >= lim) return false;
  a.end[i] = (int)ntasks;
  return true;
}

// set(q, C, g): job q's term-1 fields of Gram job g, from the filled projection block C
template <class Job, class Term1>
static int inf_tiled(const Job* jobs, int njobs, int64_t nb, int nc, int accumulate, float* cov, void* workspace,
                     size_t workspace_bytes, hipStream_t s, bool outer, bool (*ok)(const Job&), Term1 set) {
  if (!inf_tiled_call_ok(jobs, njobs) || !cov) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i)
    if (!ok(jobs[i])) return KFAC_EINVAL;
  const int64_t rows = tiled_rows(nb, nc);
  if (!rows || tiled_npairs(nc) >= ((int64_t)1 << 31)) return KFAC_EINVAL;
  const bool have = workspace && workspace_bytes >= inf_tiled_bytes(jobs, njobs, nb, nc);
  InfArgs pa{};
  InfTiledArgs args{};
  pa.njobs = args.njobs = njobs;
  pa.nc = args.nc = nc;
  pa.nb = args.nb = nb;
  pa.rows = (int)rows;
  args.accumulate = accumulate;
  args.npairs = (int)tiled_npairs(nc);
  args.cov = cov;
  char* ws = have ? (char*)workspace : nullptr;
  int64_t n[3] = {0, 0, 0}, ng = 0;
  for (int i = 0; i < njobs; ++i) {
    const Job& q = jobs[i];
    const InfDims d = inf_dims(q, nb, nc);
    inf_set_operands(pa.job[i], q);
    int64_t hcols, hm, hn;
    inf_h_shape(q, nb, nc, hcols, hm, hn);
    if (!inf_fill_proj(pa, i, d, hcols, hm, hn, ws, n)) return KFAC_EINVAL;
    if (!inf_tiled_add_job(args, i, d.k1, d.ra * d.rg, ng)) return KFAC_EINVAL;
    if (ws) {
      InfTiledJobDev& g = args.x[i];
      g.Y = pa.job[i].Y;
      g.part1 = reinterpret_cast<float*>(ws); ws += inf_tiled_partial_bytes(nb, nc, d.k1);
      g.part2 = reinterpret_cast<float*>(ws); ws += inf_tiled_partial_bytes(nb, nc, d.ra * d.rg);
      set(q, pa.job[i], g);
    }
  }
  if (!have) return KFAC_EWORKSPACE;
  const int rc = inf_launch_proj(pa, outer, n, s);
  if (rc != KFAC_OK) return rc;
  hipLaunchKernelGGL(kfac_inf_tiled_gram, dim3((unsigned)ng), dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  const dim3 grid((unsigned)(args.nb * args.npairs), JTILE2 / NTHREADS);
  hipLaunchKernelGGL(kfac_inf_tiled_reduce, grid, dim3(NTHREADS), 0, s, args);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

}  // namespace kfac

using namespace kfac;

extern "C" size_t kfac_inf_cov_tiled_workspace_bytes(const kfac_inf_cov_job* jobs, int njobs, int64_t nb,
                                                     int nc) {
  return inf_tiled_bytes(jobs, njobs, nb, nc);
}

extern "C" int kfac_inf_cov_tiled(const kfac_inf_cov_job* jobs, int njobs, int64_t nb, int nc, int accumulate,
                                  float* cov, void* workspace, size_t workspace_bytes, kfac_stream_t stream) {
  return inf_tiled<kfac_inf_cov_job>(jobs, njobs, nb, nc, accumulate, cov, workspace, workspace_bytes,
                                     (hipStream_t)stream, false, inf_job_ok,
                                     [](const kfac_inf_cov_job& q, const InfJobDev&, InfTiledJobDev& g) {
                                       g.R = q.J; g.ldR = q.ldJ;
                                       g.w = q.W; g.stride_b = 0;
                                     });
}

extern "C" size_t kfac_inf_cov_outer_tiled_workspace_bytes(const kfac_inf_cov_outer_job* jobs, int njobs,
                                                           int64_t nb, int nc) {
  return inf_tiled_bytes(jobs, njobs, nb, nc);
}

extern "C" int kfac_inf_cov_outer_tiled(const kfac_inf_cov_outer_job* jobs, int njobs, int64_t nb, int nc,
                                        int accumulate, float* cov, void* workspace, size_t workspace_bytes,
                                        kfac_stream_t stream) {
  return inf_tiled<kfac_inf_cov_outer_job>(
      jobs, njobs, nb, nc, accumulate, cov, workspace, workspace_bytes, (hipStream_t)stream, true,
      inf_outer_job_ok, [](const kfac_inf_cov_outer_job& q, const InfJobDev& C, InfTiledJobDev& g) {
        // rho_b: row ra of sample b's (ra + 1) x nG block of HR
        g.R = q.D; g.ldR = q.ldD;
        g.w = C.HX + (int64_t)q.ra * q.nG; g.stride_b = ((int64_t)q.ra + 1) * q.nG;
      });
}
