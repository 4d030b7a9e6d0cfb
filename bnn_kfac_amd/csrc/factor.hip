// Kronecker-factor accumulation (KFAC.update) on gfx950.
//
// Replaces models/curvatures.py:341-363: per layer A = [a 1]^T[a 1]/cols and
// G = g^T g/cols (Conv2d through an implicit im2col / channel-major view instead
// of F.unfold + permute().contiguous() copies), then state = state + factor.
//
// One KFAC.update() = two launches per launch group (all row-major factors together,
// each conv factor on its own):
//   1. the group's factor kernel: split-K partial products, each task writing 64x64 fp32
//      partial slabs (deterministic, no atomics).  One kernel family per file,
//      factor_<family>.hip; route_group() below picks the family, once per launch;
//   2. kfac_factor_reduce (factor_tiles.hip): per tile, sum the slabs in split order,
//      apply F = beta*F + alpha*sum, write the tile and its mirror.
// This file is the host side only: job helpers, the router, the K-split planner, the
// launch sequence and the C entry points.
#include <algorithm>
#include <utility>
#include <vector>

#include "factor_common.h"

namespace kfac {

struct Plan {
  int tiles, splits;  // splits: slabs per tile
  int units;  // workgroups per K-split: tiles, or a staged conv job's block groups
  int tasks;  // workgroups of the job
  int64_t chunk;
  size_t slab_bytes;
};

static int factor_n(const kfac_factor_job& j) { return j.x.cols + (j.x.has_ones ? 1 : 0); }

// K stages (BK rows each, never straddling two batches) of a job.
static int64_t job_sps(const kfac_factor_job& j) { return std::max<int64_t>(1, cdiv(j.x.rows, BK)); }
static int job_nseg(const kfac_factor_job& j) { return j.nseg > 1 ? j.nseg : 1; }
// a multi-batch job whose last batch is shorter (x.last_rows)
static bool job_ragged(const kfac_factor_job& j) {
  return j.nseg > 1 && j.x.last_rows > 0 && j.x.last_rows < j.x.rows;
}
static int64_t job_stages(const kfac_factor_job& j) {
  if (job_ragged(j)) return job_sps(j) * (j.nseg - 1) + std::max<int64_t>(1, cdiv(j.x.last_rows, BK));
  return job_sps(j) * job_nseg(j);
}
// K rows of a job (every batch; conv operands: images x positions) -- the profile's work
static int64_t job_krows(const kfac_factor_job& j) {
  if (job_ragged(j)) return j.x.rows * (j.nseg - 1) + j.x.last_rows;
  return j.x.rows * job_nseg(j);
}
// algorithmic bytes of a job's operand, read once: rows x cols x 4 (row-major, and the
// channel-major grads: images x positions x channels), the images themselves for the
// implicit im2col (images x C x H x W x 4)
static double job_operand_bytes(const kfac_factor_job& j) {
  const double rows = (double)job_krows(j);
  if (j.x.layout == KFAC_PATCH)
    return rows / (double)std::max<int64_t>(1, j.x.L) * (double)j.x.C * j.x.H * j.x.W * sizeof(float);
  return rows * j.x.cols * sizeof(float);
}

// Row-major operand with 16-byte-aligned rows: the LDS-DMA paths.
static bool job_glds(const kfac_factor_job& jb) {
  if (!(jb.x.layout == KFAC_ROWMAJOR && jb.x.rows > 0 && jb.x.cols >= 4 && (jb.x.cols % 4) == 0 &&
        (jb.x.ld % 4) == 0 && (reinterpret_cast<uintptr_t>(jb.x.ptr) % 16) == 0))
    return false;
  if (jb.nseg > 1 && jb.seg_ptrs) {  // (16-byte pieces start at every batch base)
    const uintptr_t* bases = reinterpret_cast<const uintptr_t*>(jb.seg_ptrs);
    for (int s = 0; s < jb.nseg; ++s)
      if (bases[s] % 16) return false;
  }
  return true;
}

// ------------------------------------------------------------------- routing
// The kernel family of a launch group: decided once per launch (route_group) and handed
// to the planner, the argument builder and the launch.  `family` is the family's profile
// slot (kfac_prof_id: the kernel name rocprofv3 reports); `cg` is the job's geometry on
// the conv families, whose tasks own whole images.
struct Route {
  int family;
  ConvGeom cg;
};

struct Family {
  int id;       // kfac_prof_id
  int wgs;      // resident workgroups per CU the planner counts on
  bool images;  // a conv family: one job per launch, geometry in Route::cg
  int (*launch)(const FactorArgs&, const ConvGeom&, int tasks, hipStream_t);
};

static const Family FAMILIES[] = {
    {KFAC_PROF_FACTOR_TILES, TILES_WGS, false,
     [](const FactorArgs& a, const ConvGeom&, int t, hipStream_t s) { return launch_tiles(a, t, s); }},
    {KFAC_PROF_FACTOR_SYRK3, S3D_WGS, false,
     [](const FactorArgs& a, const ConvGeom&, int t, hipStream_t s) { return launch_syrk3(a, t, s); }},
    {KFAC_PROF_FACTOR_X3, X3_WGS, false,
     [](const FactorArgs& a, const ConvGeom&, int t, hipStream_t s) { return launch_tiles_x3(a, t, s); }},
    {KFAC_PROF_FACTOR_CONV, KFAC_CONV_OCC, true, launch_conv},
    {KFAC_PROF_FACTOR_CONV_X3, CONV_X3_WGS, true, launch_conv_x3},
    {KFAC_PROF_FACTOR_CONV_X3S, CONV_X3_WGS, true, launch_conv_x3s},
    {KFAC_PROF_FACTOR_CONV_X3F, CONV_X3_WGS, true, launch_conv_x3f},
    {KFAC_PROF_FACTOR_CHANNEL_X3, CHANNEL_WGS, true, launch_channel_x3},
    {KFAC_PROF_FACTOR_CHANNEL_SMALL, CHANNEL_WGS, true, launch_channel_small},
};

static const Family& family_of(const Route& r) {
  for (const Family& f : FAMILIES)
    if (f.id == r.family) return f;
  return FAMILIES[0];
}

// A row-major group the bf16x3 SYRK kernels can read (buffer loads): every job either
// LDS-eligible (16-byte rows) or narrow (n <= 32, direct loads), a batch's bytes one
// 31-bit record range.  Returns the group's largest factor order, 0 when not eligible.
static int x3_eligible_nmax(const kfac_factor_job* jobs, int njobs) {
  int nmax = 0;
  for (int i = 0; i < njobs; ++i) {
    if (jobs[i].x.layout != KFAC_ROWMAJOR) return 0;
    const int n = factor_n(jobs[i]);
    if (n > 32 && !job_glds(jobs[i])) return 0;
    if (n > 32 && jobs[i].x.rows * jobs[i].x.ld * (int64_t)sizeof(float) >= ((int64_t)1 << 31)) return 0;
    nmax = std::max(nmax, n);
  }
  return nmax;
}

// bf16x3 SYRK (kfac_factor_syrk3) for a row-major launch group.
// Default: a group whose largest factor has n >= 2048 (measured A/B, same box: wide
// MLP 4097^2 factors 1.17e6 vs 9.4e5 img/s; the MNIST MLP's n <= 785 8.1e7 vs 1.0e8
// -- there the split pass's padded 6-byte images (785 -> 896, 129 -> 256 columns)
// cost as much as the fp32 kernel's whole launch).  KFAC_SYRK3=1 / 0 forces it.
static bool syrk3_group(const kfac_factor_job* jobs, int njobs) {
  const int knob = knobs().syrk3;
  if (knob == 0) return false;
  const int nmax = x3_eligible_nmax(jobs, njobs);
  return nmax > 32 && (knob == 1 || nmax >= 2048);
}

// kfac_factor_tiles_x3 (fp32 panels, bf16x3 products split in registers) for every
// row-major group kfac_factor_syrk3 does not take (default; KFAC_TILES_X3=0: the
// fp32-MFMA kfac_factor_tiles).  MNIST MLP, same box, 2 reps: 1.21-1.23e8 vs
// 1.01e8 img/s, 81-82 vs 108 us per launch, the inversion beside the pass 0.41 vs
// 0.61 ms (2 SYRK waves per SIMD instead of 4).  Groups whose largest factor has
// n < 256 keep the fp32 kernel.  LeNet-5's fully connected factors (n <= 401) measured
// 1.34e7 vs 1.39e7 img/s with x3 in round 5; with round 6's conv kernels the pass is
// 2.01-2.02 vs 2.06 ms with x3 (0.26 vs 0.31 ms of fc factors, 3 reps alternating,
// `profiles/r06z13/`), so the threshold moved from 512 to 256.
// A group whose largest factor has more than X3_PMAX panels (n > 2048: with
// kfac_factor_syrk3 switched off), or whose distinct unit tables do not fit one launch's
// arguments, keeps the fp32 kernel too.
static bool tiles_x3_group(const kfac_factor_job* jobs, int njobs) {
  const int knob = knobs().tiles_x3;
  const int nmax = x3_eligible_nmax(jobs, njobs);
  if (knob == 0 || nmax < (knob == 1 ? 33 : 256) || x3_panels(nmax) > X3_PMAX) return false;
  int n[MAXJ];
  for (int i = 0; i < njobs; ++i) n[i] = factor_n(jobs[i]);
  return x3_table_entries(n, njobs) <= X3_UCAP;
}

// A conv job on a kernel whose tasks own whole images: its family and geometry into `r`.
// false: the job takes the register-staged kfac_factor_tiles (images too large, channel
// blocks not float4-shaped, or an empty batch), one batch per launch.  A multi-batch
// job's images are its nseg batches' images in order.
static bool conv_geom(const kfac_factor_job& j, Route& r) {
  const kfac_operand& o = j.x;
  const int64_t nseg = job_nseg(j);
  if ((o.layout != KFAC_PATCH && o.layout != KFAC_CHANNEL) || o.rows <= 0 || o.L <= 0 ||
      o.rows % o.L != 0 || nseg * (o.rows / o.L) > (1 << 30))
    return false;
  // (a CHANNEL operand with a ones column -- legal, unused by the hooks -- takes the
  // unstaged kernel: the channel kernels have no ones row)
  if (o.layout == KFAC_CHANNEL && o.has_ones) return false;
  ConvGeom& g = r.cg;
  g = ConvGeom{};
  g.n = factor_n(j);
  g.ones = o.has_ones ? o.cols : -1;
  g.bseg = (int)(o.rows / o.L);
  g.B = (int)(nseg * g.bseg);
  if (o.layout == KFAC_PATCH && knobs().conv_x3) {
    const int x3 = conv_x3s_geom(o, g)   ? KFAC_PROF_FACTOR_CONV_X3S
                   : conv_x3f_geom(o, g) ? KFAC_PROF_FACTOR_CONV_X3F
                   : conv_x3_geom(o, g)  ? KFAC_PROF_FACTOR_CONV_X3 : -1;
    if (x3 >= 0) {
      r.family = x3;
      return true;
    }
  }
  // a multi-batch CHANNEL job's float4 image loads start at every batch base (seg_ptrs
  // is a host table): one misaligned base sends the job to the per-batch launches
  if (o.layout == KFAC_CHANNEL && nseg > 1) {
    const uintptr_t* bases = reinterpret_cast<const uintptr_t*>(j.seg_ptrs);
    for (int64_t s = 0; s < nseg; ++s)
      if (bases[s] % 16 != 0) return false;
  }
  if (!conv_fp32_geom(o, g)) return false;
  r.family = o.layout != KFAC_CHANNEL ? KFAC_PROF_FACTOR_CONV
             : channel_small(g)       ? KFAC_PROF_FACTOR_CHANNEL_SMALL
             : channel_x3_geom(o, g)  ? KFAC_PROF_FACTOR_CHANNEL_X3 : KFAC_PROF_FACTOR_CONV;
  return true;
}

// launch_groups() gives every channel-major / im2col job a group of its own.
static Route route_group(const kfac_factor_job* jobs, int njobs) {
  Route r{};
  r.family = KFAC_PROF_FACTOR_TILES;
  if (syrk3_group(jobs, njobs))
    r.family = KFAC_PROF_FACTOR_SYRK3;
  else if (tiles_x3_group(jobs, njobs))
    r.family = KFAC_PROF_FACTOR_X3;
  else if (njobs == 1)
    conv_geom(jobs[0], r);
  return r;
}

// ------------------------------------------------------------------ K-split plan
// Split K so that the grouped launch fills the chip's workgroup slots (256 CUs x the
// family's resident workgroups) in as few dispatch rounds as possible with every task
// still running >= 8 stages (256 rows) of MFMA work.  One chunk length c (stages) is used
// for every job; tasks(c) = sum_j tiles_j * ceil(stages_j / c) falls with c, and the
// modelled time is (c + prologue/epilogue) * rounds: the smallest c that fits r
// rounds is found by bisection for r = 1..4 and the cheapest r wins.
// A job with a deferred-reduction accumulator keeps the accumulator's split count
// (its layout): its stage range is cut into that many equal chunks (trailing splits
// of a smaller batch may be empty and then contribute zero).
static void plan_jobs(const kfac_factor_job* jobs, int njobs, const Route& route, Plan* plans) {
  const Family& fam = family_of(route);
  const bool s3 = route.family == KFAC_PROF_FACTOR_SYRK3, x3 = route.family == KFAC_PROF_FACTOR_X3;
  const int64_t slots = (int64_t)fam.wgs * 256;
  constexpr int64_t MIN_CHUNK = 8, OVERHEAD = 4;  // stages; ~per-task fixed cost in stages
  int64_t max_steps = 1;
  for (int i = 0; i < njobs; ++i) max_steps = std::max(max_steps, job_stages(jobs[i]));
  int64_t units[MAXJ];
  for (int i = 0; i < njobs; ++i) {
    const int n = factor_n(jobs[i]);
    const int64_t t = cdiv(n, TILE);
    units[i] = s3 ? syrk3_units(n) : x3 ? x3_units(n) : fam.images ? route.cg.units : t * (t + 1) / 2;
  }
  // a factor whose last 64-column tile row holds one 32-column panel (the MNIST MLP's 785
  // and 129): see max_rounds below
  auto thin = [&](int i) {
    const int n = factor_n(jobs[i]);
    return x3 && n > TILE && (n - 1) % TILE < 32;
  };
  // workgroups of job i at `splits` slabs per tile
  auto job_tasks = [&](int i, int64_t splits) { return units[i] * splits; };
  // (kfac_factor_tiles_x3: narrow jobs (n <= 32) at 4x the chunk's K-splits measured ~1 %
  // slower on the MLP line, profiles/r04ah/)
  auto job_splits = [&](int i, int64_t c) { return cdiv(job_stages(jobs[i]), c); };
  auto tasks_at = [&](int64_t c) {
    int64_t n = 0;
    for (int i = 0; i < njobs; ++i)
      n += job_tasks(i, job_splits(i, c));
    return n;
  };
  int64_t best_c = std::max(MIN_CHUNK, max_steps), best_cost = -1;
  // (kfac_factor_tiles_x3 groups with such a factor: one round -- MNIST MLP, same box:
  // 163.4 vs 170.3 / 167.4 us per launch at the two rounds the cost model picks, measured
  // on the 64 x 64 tile units this kernel had before its panel cliques and not again
  // since; other x3 groups keep the cost model's choice, which nothing measured against)
  bool any_thin = false;
  for (int i = 0; i < njobs; ++i) any_thin |= thin(i);
  // (kfac_factor_syrk3 groups, 2 workgroups per CU: up to 16 rounds, so a launch of
  // ~2,200 macro tiles (wide C5) can take 2 K-splits at 9 rounds instead of 1 at 4.3:
  // 1.61 vs 1.71 ms per launch, profiles/r05ac/)
  const int64_t max_rounds = any_thin ? 1 : (s3 ? 16 : 4);
  for (int64_t r = 1; r <= max_rounds; ++r) {
    int64_t lo = MIN_CHUNK, hi = std::max(MIN_CHUNK, max_steps);
    if (tasks_at(hi) > r * slots) continue;  // even one split per tile needs more rounds
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (tasks_at(mid) <= r * slots) hi = mid; else lo = mid + 1;
    }
    const int64_t cost = (lo + OVERHEAD) * r;
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_c = lo; }
  }
  for (int i = 0; i < njobs; ++i) {
    const int t = (int)cdiv(factor_n(jobs[i]), TILE);
    Plan& p = plans[i];
    p.tiles = t * (t + 1) / 2;
    p.units = (int)units[i];
    const int64_t steps = job_stages(jobs[i]);
    if (jobs[i].acc) {
      p.splits = jobs[i].acc_splits;
      p.chunk = cdiv(steps, (int64_t)p.splits);
      p.slab_bytes = 0;  // partials go to the caller's accumulator
      p.tasks = (int)job_tasks(i, p.splits);
      continue;
    }
    p.splits = (int)job_splits(i, best_c);
    if (fam.images) {
      // Tasks own whole images, the SAME number k each, and fill the resident slots
      // once: k = the fewest images per task that keep units x ceil(B / k) tasks
      // within the slots.  A workgroup's time is k times a per-image cost, so a mix of
      // 2- and 3-image tasks waited on the 3-image ones, and a CU running more
      // workgroups than another finished later (LeNet-5, batch 1024: conv2 A 68 us at
      // 400 splits -> 53 us at k = 2 (1,024 tasks); conv1 A 34 -> 27 us at k = 1;
      // `git show e37cdaa^:tools/microbench/conv_ab.hip`, KFAC_CONV_K overrides k)
      const ConvGeom& cg = route.cg;
      // (the n <= 8 channel kernel: half the slots -- its per-task reduction is the
      // larger cost there: conv1 G 15.7 / 12.4 / 13.2 us at k = 1 / 2 / 4 -- unless a
      // multi-batch launch -- thousands of images -- amortizes that reduction: the kernel
      // then takes 4 workgroups per CU, twice the loads in flight of 2)
      const bool halve = route.family == KFAC_PROF_FACTOR_CHANNEL_SMALL && cg.B <= 8 * slots;
      int k = (int)std::max<int64_t>(1, cdiv((int64_t)cg.units * cg.B, halve ? slots / 2 : slots));
      if (knobs().conv_k > 0) k = knobs().conv_k;
      k = std::min(k, cg.B);
      p.splits = (int)cdiv(cg.B, k);
    }
    p.chunk = cdiv(steps, (int64_t)p.splits);
    p.slab_bytes = align_up((size_t)p.tiles * p.splits * TILE * TILE * sizeof(float), 256);
    p.tasks = (int)job_tasks(i, p.splits);
  }
}

static size_t accum_bytes(int n, int splits) {
  const int64_t t = cdiv(n, TILE);
  return align_up((size_t)(t * (t + 1) / 2) * splits * TILE * TILE * sizeof(float), 256);
}

static bool valid_operand(const kfac_operand& o) {
  if (o.cols < 0 || o.rows < 0 || (!o.ptr && o.rows > 0)) return false;
  switch (o.layout) {
    case KFAC_ROWMAJOR: return o.ld >= o.cols;
    case KFAC_CHANNEL: return o.L > 0 && o.sB >= 0;
    case KFAC_PATCH:
      return o.L > 0 && o.C > 0 && o.H > 0 && o.W > 0 && o.kh > 0 && o.kw > 0 && o.sh > 0 &&
             o.sw > 0 && o.ph >= 0 && o.pw >= 0 && o.Ho > 0 && o.Wo > 0 &&
             (int64_t)o.Ho * o.Wo == o.L && o.cols == o.C * o.kh * o.kw && o.kh < 65536 &&
             o.kw < 65536;
    default: return false;
  }
}

static void fill_dev(FactorJobDev& d, const kfac_factor_job& jb) {
  d.x = to_dev(jb.x);
  d.alpha = jb.alpha;
  d.beta = jb.beta;
  d.F = jb.F;
  d.ldF = jb.ldF;
  d.n = factor_n(jb);
  d.t = (int)cdiv(d.n, TILE);
  d.accum = jb.acc != nullptr;
  d.sbeta = jb.acc_beta;
  d.seg_off = -1;  // prepare_group() places multi-batch bases
  d.nseg = job_nseg(jb);
  d.sps = (int)job_sps(jb);
  d.nst = job_stages(jb);
  d.rstage = -1;
  d.rw = d.rinv = 1.f;
  d.rdelta = 0;
  if (job_ragged(jb)) {
    d.rdelta = (int)(jb.x.rows - jb.x.last_rows);
    d.rstage = (int64_t)d.sps * (jb.nseg - 1);
    d.rw = (float)((double)jb.x.rows / (double)jb.x.last_rows);
    d.rinv = (float)((double)jb.x.last_rows / (double)jb.x.rows);
  }
}

// The launch arguments of one grouped update: the family's launch (`args`, `tasks`
// workgroups) and the reduce of the jobs without an accumulator (`red`, `rtiles`
// tiles).  Returns KFAC_EWORKSPACE when the slabs do not fit.
struct GroupLaunch {
  FactorArgs args, red;
  int tasks, rtiles;
};

static int prepare_group(const kfac_factor_job* jobs, int njobs, const Route& route, char* ws,
                         size_t ws_bytes, GroupLaunch& g) {
  Plan plans[MAXJ];
  plan_jobs(jobs, njobs, route, plans);
  FactorArgs& args = g.args;
  FactorArgs& red = g.red;  // the reduce launch: jobs reduced now (no accumulator)
  args = FactorArgs{};
  red = FactorArgs{};
  args.njobs = njobs;
  // split-major task order (each XCD a contiguous range of K-splits of all tiles):
  // 55 k vs 194 k KiB fetched per launch tile-major at equal time
  args.split_major = 1;
  int tasks = 0, rtiles = 0, nsegs = 0;
  size_t off = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_factor_job& jb = jobs[i];
    FactorJobDev& d = args.job[i];
    fill_dev(d, jb);
    d.glds = job_glds(jb);
    d.x3units = route.family == KFAC_PROF_FACTOR_X3 ? plans[i].units : 0;  // (x3tab: launch_tiles_x3)
    d.splits = plans[i].splits;
    d.sstride = jb.acc && jb.acc_stride > 0 ? jb.acc_stride : d.splits;
    d.chunk = plans[i].chunk;
    if (d.nseg > 1) {  // kfac_factor_update keeps a launch within KSEG batch bases
      const float* const* bases = reinterpret_cast<const float* const*>(jb.seg_ptrs);
      d.seg_off = nsegs;
      for (int s = 0; s < d.nseg; ++s) args.segs[nsegs++] = bases[s];
    }
    if (jb.acc) {
      d.slab = jb.acc;
    } else {
      d.slab = reinterpret_cast<float*>(ws + off);
      off += plans[i].slab_bytes;
      FactorJobDev& e = red.job[red.njobs];
      e = d;
      e.tile_begin = rtiles;
      rtiles += plans[i].tiles;
      red.tile_end[red.njobs++] = rtiles;
    }
    d.task_begin = tasks;
    tasks += plans[i].tasks;
    args.task_end[i] = tasks;
  }
  // kfac_factor_tiles_x3 with every job at the same K-splits (the planner's one chunk
  // length, or the callers' acc_splits): split-major across the whole launch, the task
  // ranges counted in units per split (x3_task_decode)
  if (route.family == KFAC_PROF_FACTOR_X3) {
    bool same = true;
    for (int i = 1; i < njobs; ++i) same &= args.job[i].splits == args.job[0].splits;
    if (same && args.job[0].splits > 0) {
      args.split_major = 2;
      int units = 0;
      for (int i = 0; i < njobs; ++i) {
        args.job[i].task_begin = units;
        units += args.job[i].x3units;
        args.task_end[i] = units;
      }
    }
  }
  g.tasks = tasks;
  g.rtiles = rtiles;
  return off > ws_bytes ? KFAC_EWORKSPACE : KFAC_OK;
}

// One launch group on the kernel family `route` names, then the reduce of its slabs.
static int factor_group(const kfac_factor_job* jobs, int njobs, const Route& route, char* ws,
                        size_t ws_bytes, hipStream_t stream) {
  GroupLaunch g;
  const int rc = prepare_group(jobs, njobs, route, ws, ws_bytes, g);
  if (rc != KFAC_OK) return rc;
  if (g.tasks == 0) return KFAC_OK;
  {
    // the family's profile slot, with the launch's algorithmic flops: sum over jobs of
    // K rows x n (n + 1)
    double work = 0.0, bytes = 0.0;
    if (prof_on())
      for (int i = 0; i < njobs; ++i) {
        work += (double)job_krows(jobs[i]) * factor_n(jobs[i]) * (factor_n(jobs[i]) + 1);
        bytes += job_operand_bytes(jobs[i]);
      }
    ProfScope ps(route.family, stream, work, bytes);
    // (a launcher that fails has launched nothing: no reduce over slabs no kernel wrote)
    const int lrc = family_of(route).launch(g.args, route.cg, g.tasks, stream);
    if (lrc != KFAC_OK) return lrc;
    KFAC_CHECK_LAUNCH();
  }
  launch_reduce(g.red, g.rtiles, stream);
  KFAC_CHECK_LAUNCH();
  return KFAC_OK;
}

static size_t group_ws(const kfac_factor_job* jobs, int njobs, const Route& route) {
  Plan plans[MAXJ];
  plan_jobs(jobs, njobs, route, plans);
  size_t off = 0;
  for (int i = 0; i < njobs; ++i) off += plans[i].slab_bytes;
  return off;
}

}  // namespace kfac

using namespace kfac;

// Row-major jobs share launches (up to MAXJ each): their K-steps cost alike, so the
// planner's equal-step split balances them.  Each channel-major / im2col job gets
// a launch (and a plan) of its own: a K-step of a gather-bound operand costs far
// more than one of a row-major MFMA tile, and mixing them leaves the fast tasks
// idle behind the slow ones (LeNet-5: 1.35 ms grouped vs 0.94 ms per-job).
// `order` receives the caller's job index of each entry of `sorted`.
static void launch_groups(const kfac_factor_job* jobs, int njobs, std::vector<kfac_factor_job>& sorted,
                          std::vector<int>& order, std::vector<std::pair<int, int>>& groups) {
  sorted.clear();
  order.clear();
  groups.clear();
  for (int i = 0; i < njobs; ++i)
    if (jobs[i].x.layout == KFAC_ROWMAJOR) {
      sorted.push_back(jobs[i]);
      order.push_back(i);
    }
  const int nrm = (int)sorted.size();
  for (int g = 0; g < nrm; g += MAXJ) groups.emplace_back(g, std::min(MAXJ, nrm - g));
  for (int i = 0; i < njobs; ++i)
    if (jobs[i].x.layout != KFAC_ROWMAJOR) {
      groups.emplace_back((int)sorted.size(), 1);
      sorted.push_back(jobs[i]);
      order.push_back(i);
    }
}

extern "C" size_t kfac_factor_workspace_bytes(const kfac_factor_job* jobs, int njobs) {
  if (!jobs || njobs <= 0) return 0;
  std::vector<kfac_factor_job> sorted;
  std::vector<int> order;
  std::vector<std::pair<int, int>> groups;
  launch_groups(jobs, njobs, sorted, order, groups);
  size_t m = 0;
  for (const auto& g : groups) {
    const kfac_factor_job* gj = sorted.data() + g.first;
    m = std::max(m, group_ws(gj, g.second, route_group(gj, g.second)));
  }
  return m;
}

static int validate(const kfac_factor_job* jobs, int njobs) {
  if (njobs < 0 || (njobs > 0 && !jobs)) return KFAC_EINVAL;
  for (int i = 0; i < njobs; ++i) {
    const kfac_factor_job& j = jobs[i];
    if (!valid_operand(j.x) || !j.F || j.ldF < factor_n(j)) return KFAC_EINVAL;
    if ((int64_t)factor_n(j) > (int64_t)1 << 20) return KFAC_EINVAL;
    if (j.acc && (j.acc_splits <= 0 || j.acc_splits > (1 << 20))) return KFAC_EINVAL;
    if (j.acc && j.acc_stride != 0 && (j.acc_stride < j.acc_splits || j.acc_stride > (1 << 20)))
      return KFAC_EINVAL;
    if (j.nseg < 0 || (j.nseg > 1 && !j.seg_ptrs) || job_sps(j) > (1 << 30))
      return KFAC_EINVAL;
    if (j.x.last_rows < 0 || j.x.last_rows > j.x.rows ||
        (job_ragged(j) && j.x.layout != KFAC_ROWMAJOR))
      return KFAC_EINVAL;
  }
  return KFAC_OK;
}

extern "C" int kfac_factor_accum_plan(const kfac_factor_job* jobs, int njobs, int32_t* splits,
                                      size_t* bytes) {
  if (validate(jobs, njobs) != KFAC_OK || (njobs > 0 && (!splits || !bytes))) return KFAC_EINVAL;
  std::vector<kfac_factor_job> sorted;
  std::vector<int> order;
  std::vector<std::pair<int, int>> groups;
  launch_groups(jobs, njobs, sorted, order, groups);
  for (auto& j : sorted) j.acc = nullptr;  // plan as an immediate update of this batch
  for (const auto& g : groups) {
    Plan plans[MAXJ];
    const kfac_factor_job* gj = sorted.data() + g.first;
    plan_jobs(gj, g.second, route_group(gj, g.second), plans);
    for (int k = 0; k < g.second; ++k) {
      const int i = order[g.first + k];
      splits[i] = plans[k].splits;
      bytes[i] = accum_bytes(factor_n(jobs[i]), plans[k].splits);
    }
  }
  return KFAC_OK;
}

extern "C" int kfac_factor_route(const kfac_factor_job* jobs, int njobs, int32_t* family) {
  if (validate(jobs, njobs) != KFAC_OK || (njobs > 0 && !family)) return KFAC_EINVAL;
  std::vector<kfac_factor_job> sorted;
  std::vector<int> order;
  std::vector<std::pair<int, int>> groups;
  launch_groups(jobs, njobs, sorted, order, groups);
  for (const auto& g : groups) {
    const int fam = route_group(sorted.data() + g.first, g.second).family;
    for (int k = 0; k < g.second; ++k) family[order[g.first + k]] = fam;
  }
  return KFAC_OK;
}

// One launch group of kfac_factor_update: routed here, and routed again for every group
// this function rewrites.  A ragged multi-batch job (x.last_rows) runs in one launch on
// kfac_factor_tiles_x3 (and its narrow tasks); any other kernel, or a group past the
// launch's KSEG batch bases, takes it as two launches: the equal batches, then the last
// batch as a job of its own (alpha * rows / last_rows, adding).
static int update_group(const kfac_factor_job* gj, int n, void* workspace, size_t workspace_bytes,
                        kfac_stream_t stream) {
  bool ragged = false;
  int nbases = 0;
  for (int k = 0; k < n; ++k) {
    ragged |= job_ragged(gj[k]);
    nbases += job_nseg(gj[k]) > 1 ? gj[k].nseg : 0;
  }
  const Route route = route_group(gj, n);
  if (ragged && (route.family != KFAC_PROF_FACTOR_X3 || nbases > KSEG)) {
    std::vector<kfac_factor_job> head(gj, gj + n), tail;
    for (kfac_factor_job& j : head) {
      if (!job_ragged(j)) continue;
      const float* const* bases = reinterpret_cast<const float* const*>(j.seg_ptrs);
      kfac_factor_job t = j;
      t.x.ptr = bases[j.nseg - 1];
      t.x.rows = j.x.last_rows;
      t.x.last_rows = 0;
      t.seg_ptrs = nullptr;
      t.nseg = 0;
      t.alpha = (float)((double)j.alpha * (double)j.x.rows / (double)j.x.last_rows);
      if (t.acc) t.acc_beta = 1.f;
      else t.beta = 1.f;
      tail.push_back(t);
      j.x.last_rows = 0;
      if (--j.nseg == 1) {
        j.x.ptr = bases[0];
        j.seg_ptrs = nullptr;
        j.nseg = 0;
      }
    }
    int rc = update_group(head.data(), n, workspace, workspace_bytes, stream);
    if (rc != KFAC_OK) return rc;
    return update_group(tail.data(), (int)tail.size(), workspace, workspace_bytes, stream);
  }
  if (n == 1 && gj[0].x.layout != KFAC_ROWMAJOR && job_nseg(gj[0]) > 1 && !family_of(route).images) {
    // a multi-batch conv job off the image-staged kernels (images too large for LDS):
    // the register-staged kernels read one batch base, so one launch per batch,
    // each adding to what the previous one wrote
    const float* const* bases = reinterpret_cast<const float* const*>(gj[0].seg_ptrs);
    for (int s = 0; s < gj[0].nseg; ++s) {
      kfac_factor_job j = gj[0];
      j.seg_ptrs = nullptr;
      j.nseg = 0;
      j.x.ptr = bases[s];
      if (s > 0) {
        if (j.acc) j.acc_beta = 1.f;
        else j.beta = 1.f;
      }
      const int rc = factor_group(&j, 1, route_group(&j, 1), (char*)workspace, workspace_bytes,
                                  (hipStream_t)stream);
      if (rc != KFAC_OK) return rc;
    }
    return KFAC_OK;
  }
  int multi = 0, maxseg = 1, total = 0;
  for (int k = 0; k < n; ++k)
    if (job_nseg(gj[k]) > 1) {
      ++multi;
      maxseg = std::max(maxseg, gj[k].nseg);
      total += gj[k].nseg;
    }
  if (total <= KSEG)
    return factor_group(gj, n, route, (char*)workspace, workspace_bytes, (hipStream_t)stream);
  // more batch bases than one launch's kernel arguments hold: rounds of S batches
  // per multi-batch job, each round adding to what the previous ones wrote
  const int S = KSEG / multi;  // >= KSEG / MAXJ = 4
  for (int r = 0; r * S < maxseg; ++r) {
    std::vector<kfac_factor_job> sub;
    for (int k = 0; k < n; ++k) {
      kfac_factor_job j = gj[k];
      if (job_nseg(j) > 1) {
        const int b0 = r * S;
        if (b0 >= j.nseg) continue;
        const float* const* bases = reinterpret_cast<const float* const*>(j.seg_ptrs) + b0;
        j.seg_ptrs = bases;
        j.nseg = std::min(S, j.nseg - b0);
        j.x.ptr = bases[0];
      } else if (r > 0) {
        continue;
      }
      if (r > 0) {
        if (j.acc) j.acc_beta = 1.f;
        else j.beta = 1.f;
      }
      sub.push_back(j);
    }
    const int rc = factor_group(sub.data(), (int)sub.size(), route_group(sub.data(), (int)sub.size()),
                                (char*)workspace, workspace_bytes, (hipStream_t)stream);
    if (rc != KFAC_OK) return rc;
  }
  return KFAC_OK;
}

extern "C" int kfac_factor_update(const kfac_factor_job* jobs, int njobs, void* workspace,
                                  size_t workspace_bytes, kfac_stream_t stream) {
  const int rc0 = validate(jobs, njobs);
  if (rc0 != KFAC_OK) return rc0;
  // Launch groups run back to back on the stream, reusing the same workspace.
  std::vector<kfac_factor_job> sorted;
  std::vector<int> order;
  std::vector<std::pair<int, int>> groups;
  launch_groups(jobs, njobs, sorted, order, groups);
  for (const auto& g : groups) {
    const int rc = update_group(sorted.data() + g.first, g.second, workspace, workspace_bytes, stream);
    if (rc != KFAC_OK) return rc;
  }
  return KFAC_OK;
}

extern "C" int kfac_factor_flush(const kfac_factor_job* jobs, int njobs, kfac_stream_t stream) {
  const int rc0 = validate(jobs, njobs);
  if (rc0 != KFAC_OK) return rc0;
  FactorArgs red{};
  int tiles = 0;
  for (int i = 0; i < njobs; ++i) {
    const kfac_factor_job& jb = jobs[i];
    if (!jb.acc) return KFAC_EINVAL;
    FactorJobDev& e = red.job[red.njobs];
    fill_dev(e, jb);
    e.slab = jb.acc;
    e.splits = jb.acc_splits;
    e.sstride = jb.acc_stride > 0 ? jb.acc_stride : jb.acc_splits;
    e.tile_begin = tiles;
    tiles += e.t * (e.t + 1) / 2;
    red.tile_end[red.njobs++] = tiles;
    if (red.njobs == MAXJ || i == njobs - 1) {
      launch_reduce(red, tiles, (hipStream_t)stream);
      KFAC_CHECK_LAUNCH();
      red = FactorArgs{};
      tiles = 0;
    }
  }
  return KFAC_OK;
}

static kfac_operand rowmajor(const float* x, int64_t rows, int64_t cols, int64_t ld, int ones) {
  kfac_operand o{};
  o.ptr = x;
  o.layout = KFAC_ROWMAJOR;
  o.rows = rows;
  o.cols = (int32_t)cols;
  o.ld = ld;
  o.has_ones = ones;
  return o;
}

static int single(const kfac_operand& o, float alpha, float beta, float* F, int64_t ldF, void* ws,
                  size_t wsb, kfac_stream_t s) {
  kfac_factor_job j{};
  j.x = o;
  j.alpha = alpha;
  j.beta = beta;
  j.F = F;
  j.ldF = ldF;
  if (wsb < kfac_factor_workspace_bytes(&j, 1)) return KFAC_EWORKSPACE;
  return kfac_factor_update(&j, 1, ws, wsb, s);
}

extern "C" int kfac_syrk_linear(const float* x, int64_t B, int64_t d, int64_t ldx, int has_ones,
                                float alpha, float beta, float* F, int64_t ldF, void* ws,
                                size_t wsb, kfac_stream_t s) {
  return single(rowmajor(x, B, d, ldx, has_ones ? 1 : 0), alpha, beta, F, ldF, ws, wsb, s);
}

extern "C" int kfac_syrk_conv(const float* x, int64_t B, int C, int H, int W, int kh, int kw,
                              int sh, int sw, int ph, int pw, int has_ones, float alpha, float beta,
                              float* F, int64_t ldF, void* ws, size_t wsb, kfac_stream_t s) {
  if (sh <= 0 || sw <= 0) return KFAC_EINVAL;
  kfac_operand o{};
  o.ptr = x;
  o.layout = KFAC_PATCH;
  o.C = C; o.H = H; o.W = W; o.kh = kh; o.kw = kw; o.sh = sh; o.sw = sw; o.ph = ph; o.pw = pw;
  o.Ho = (H + 2 * ph - kh) / sh + 1;
  o.Wo = (W + 2 * pw - kw) / sw + 1;
  o.L = (int64_t)o.Ho * o.Wo;
  o.sB = (int64_t)C * H * W;
  o.rows = B * o.L;
  o.cols = C * kh * kw;
  o.has_ones = has_ones ? 1 : 0;
  return single(o, alpha, beta, F, ldF, ws, wsb, s);
}

extern "C" int kfac_syrk_convgrad(const float* g, int64_t B, int C, int64_t L, float alpha,
                                  float beta, float* F, int64_t ldF, void* ws, size_t wsb,
                                  kfac_stream_t s) {
  kfac_operand o{};
  o.ptr = g;
  o.layout = KFAC_CHANNEL;
  o.L = L;
  o.sB = (int64_t)C * L;
  o.rows = B * L;
  o.cols = C;
  return single(o, alpha, beta, F, ldF, ws, wsb, s);
}
