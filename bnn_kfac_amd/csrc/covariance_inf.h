// What the capped INF calls (covariance_inf.hip: kfac_inf_cov, kfac_inf_cov_outer) share with
// the class-tiled ones (covariance_inf_tiled.hip) and with the INF draw calls
// (covariance_inf_draws.hip, which also runs them with rows := draws): the argument block of the projection
// launches h | x, t, y -- which run over all nb*nc rows and know nothing of a class cap --
// the job checks, the sizes of HX / T / Y, and the launch of the three projections.
#pragma once

#include "covariance_common.h"

namespace kfac {

struct InfJobDev {
  const float* a;   // outer route
  const float* D;
  const float* J;   // dense route
  const float* UA;
  const float* UG;
  const float* W;
  const float* F;
  float* HX;        // outer: HR, nb x (ra+1) x nG; dense: X, rows x ra x nG
  float* T;         // rows x r
  float* Y;         // rows x r
  float* part1;     // nb x nseg1 x nc*nc   (the capped calls' Gram partials)
  float* part2;     // nb x nseg2 x nc*nc
  int64_t lda, ldD, ldJ, ldA, ldG, ldF;
  int cols, ones, nA, nG, ra, rg, r;
  int hcols;        // columns of the h / x launch's wide operand: nb*(ra+1) / rows*nG
  int trows;        // rows*ra
  int hn, tn, yn;   // tiles along the second tile index of the h|x / t / y launch
  int nseg1, nseg2;
  int h_begin, t_begin, y_begin, g1_begin, g2_begin;
};

struct InfArgs {
  int njobs, nc, accumulate, rows;  // rows = nb*nc
  int64_t nb;
  float* cov;
  int h_end[CMAXJ], t_end[CMAXJ], y_end[CMAXJ], g1_end[CMAXJ], g2_end[CMAXJ];
  InfJobDev job[CMAXJ];
};
static_assert(sizeof(InfArgs) <= 4096, "kernel argument block");

// What both routes share once a job is reduced to (nA, nG, ra, rg): sizes of T / Y and the
// Gram partials.  hx: floats of the route's first intermediate.
struct InfDims {
  int64_t nA, nG, ra, rg, k1;  // k1: the first term's Gram length (nG, or nA*nG)
  size_t hx;
};
static inline InfDims inf_dims(const kfac_inf_cov_job& q, int64_t nb, int nc) {
  return InfDims{q.nA, q.nG, q.ra, q.rg, (int64_t)q.nA * q.nG, (size_t)(nb * nc) * (size_t)q.ra * (size_t)q.nG};
}
static inline InfDims inf_dims(const kfac_inf_cov_outer_job& q, int64_t nb, int) {
  return InfDims{(int64_t)q.cols + (q.has_ones != 0), q.nG, q.ra, q.rg, q.nG,
                 (size_t)nb * (size_t)(q.ra + 1) * (size_t)q.nG};
}
static inline size_t inf_hx_bytes(const InfDims& d) { return align_up(d.hx * sizeof(float), 256); }
static inline size_t inf_ty_bytes(const InfDims& d, int64_t rows) {
  return align_up((size_t)rows * (size_t)(d.ra * d.rg) * sizeof(float), 256);
}

static inline bool inf_job_ok(const kfac_inf_cov_job& q) {
  return q.J && q.UA && q.UG && q.W && q.F && q.nA > 0 && q.nG > 0 && q.ra > 0 && q.rg > 0 &&
         q.ldJ >= (int64_t)q.nA * q.nG && q.ldA >= q.ra && q.ldG >= q.rg && q.ldW >= (int64_t)q.nA * q.nG &&
         q.ldF >= (int64_t)q.ra * q.rg;
}
static inline bool inf_outer_job_ok(const kfac_inf_cov_outer_job& q) {
  return q.a && q.D && q.UA && q.UG && q.W && q.F && q.cols > 0 && q.nG > 0 && q.ra > 0 && q.rg > 0 &&
         q.lda >= q.cols && q.ldD >= q.nG && q.ldA >= q.ra && q.ldG >= q.rg &&
         q.ldW >= ((int64_t)q.cols + (q.has_ones != 0)) * q.nG && q.ldF >= (int64_t)q.ra * q.rg;
}

// The operands of job i's device block.
static inline void inf_set_operands(InfJobDev& C, const kfac_inf_cov_job& q) {
  C.J = q.J; C.UA = q.UA; C.UG = q.UG; C.W = q.W; C.F = q.F;
  C.ldJ = q.ldJ; C.ldA = q.ldA; C.ldG = q.ldG; C.ldF = q.ldF;
}
static inline void inf_set_operands(InfJobDev& C, const kfac_inf_cov_outer_job& q) {
  C.a = q.a; C.D = q.D; C.UA = q.UA; C.UG = q.UG; C.W = q.W; C.F = q.F;
  C.lda = q.lda; C.ldD = q.ldD; C.ldA = q.ldA; C.ldG = q.ldG; C.ldF = q.ldF;
  C.cols = q.cols; C.ones = q.has_ones ? q.cols : -1;
}
// (columns, m tiles, n tiles) of the h | x launch's wide operand
static inline void inf_h_shape(const kfac_inf_cov_job& q, int64_t nb, int nc, int64_t& hcols, int64_t& hm,
                               int64_t& hn) {
  hcols = nb * nc * q.nG;
  hm = cdiv(q.ra, TILE);
  hn = cdiv(hcols, TILE);
}
static inline void inf_h_shape(const kfac_inf_cov_outer_job& q, int64_t nb, int, int64_t& hcols, int64_t& hm,
                               int64_t& hn) {
  hcols = nb * ((int64_t)q.ra + 1);
  hm = cdiv(hcols, TILE);
  hn = cdiv(q.nG, TILE);
}

// The projection part of job i's device block: its dimensions, the task ranges of the h | x,
// t and y launches (n[0..2], running over the jobs) and, where ws is not null, its HX, T and Y
// slices.  false where a 32-bit column, row or task count would overflow.
static inline bool inf_fill_proj(InfArgs& args, int i, const InfDims& d, int64_t hcols, int64_t hm, int64_t hn,
                                 char*& ws, int64_t* n) {
  const int64_t lim = ((int64_t)1 << 31) - TILE;
  const int64_t rows = args.rows, r = d.ra * d.rg;
  if (d.nA >= lim || r >= lim || hcols >= lim || rows * d.ra >= lim) return false;
  InfJobDev& C = args.job[i];
  C.nA = (int)d.nA; C.nG = (int)d.nG; C.ra = (int)d.ra; C.rg = (int)d.rg; C.r = (int)r;
  C.hcols = (int)hcols;
  C.trows = (int)(rows * d.ra);
  C.hn = (int)hn;
  C.tn = (int)cdiv(d.rg, TILE);
  C.yn = (int)cdiv(r, TILE);
  C.h_begin = (int)n[0]; C.t_begin = (int)n[1]; C.y_begin = (int)n[2];
  n[0] += hm * hn;
  n[1] += cdiv(C.trows, TILE) * C.tn;
  n[2] += cdiv(rows, TILE) * C.yn;
  for (int k = 0; k < 3; ++k)
    if (n[k] >= lim) return false;
  args.h_end[i] = (int)n[0]; args.t_end[i] = (int)n[1]; args.y_end[i] = (int)n[2];
  if (ws) {
    C.HX = reinterpret_cast<float*>(ws); ws += inf_hx_bytes(d);
    C.T = reinterpret_cast<float*>(ws); ws += inf_ty_bytes(d, rows);
    C.Y = reinterpret_cast<float*>(ws); ws += inf_ty_bytes(d, rows);
  }
  return true;
}

// kfac_inf_h | kfac_inf_x, kfac_inf_t, kfac_inf_y (covariance_inf.hip) on a filled block:
// n[0..2] their task counts.
int inf_launch_proj(const InfArgs& args, bool outer, const int64_t* n, hipStream_t s);

}  // namespace kfac
