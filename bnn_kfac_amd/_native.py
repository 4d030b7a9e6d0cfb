"""ctypes binding of libkfac_hip.so (the C ABI declared in include/kfac_hip.h).

The product path has NO fallback: if the library is missing, fails to load, or a
tensor is not on a HIP device, the calls below raise.  Device buffers are torch
tensors (the caching allocator owns them); the stream is torch's current stream
on the tensor's device, passed to every call explicitly.
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BNN_KFAC_AMD_LIB", os.path.join(_HERE, "libkfac_hip.so"))

# enums (include/kfac_hip.h)
KFAC_OK, KFAC_EINVAL, KFAC_ELAUNCH, KFAC_EWORKSPACE = 0, -1, -2, -3
ROWMAJOR, CHANNEL, PATCH = 0, 1, 2
OUT_INV_CHOL, OUT_INVERSE = 0, 1
TRI_SYMMETRIC, TRI_LOWER = 0, 1
(PROF_FACTOR_TILES, PROF_FACTOR_REDUCE, PROF_INVERT, PROF_QUAD_TILES, PROF_FACTOR_SYRK3,
 PROF_FACTOR_X3, PROF_FACTOR_CONV, PROF_FACTOR_CHANNEL_SMALL, PROF_SYEV, PROF_FACTOR_CONV_X3,
 PROF_FACTOR_CONV_X3S, PROF_FACTOR_CONV_X3F, PROF_FACTOR_CHANNEL_X3) = range(13)
# profile slot -> the kernel family rocprofv3 names (kfac_prof_id, include/kfac_hip.h; the
# fp32 SYRK is the template kfac_factor_tiles_t<...>, named without the _t as in profiles/)
PROF_FACTOR_KERNELS = {PROF_FACTOR_TILES: "kfac_factor_tiles", PROF_FACTOR_SYRK3: "kfac_factor_syrk3",
                       PROF_FACTOR_X3: "kfac_factor_tiles_x3", PROF_FACTOR_CONV: "kfac_factor_conv",
                       PROF_FACTOR_CHANNEL_SMALL: "kfac_factor_channel_small",
                       PROF_FACTOR_CONV_X3: "kfac_factor_conv_x3", PROF_FACTOR_CONV_X3S: "kfac_factor_conv_x3s",
                       PROF_FACTOR_CONV_X3F: "kfac_factor_conv_x3f", PROF_FACTOR_CHANNEL_X3: "kfac_factor_channel_x3"}

c_i32, c_i64, c_f32, c_f64, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p


class Operand(ctypes.Structure):
    _fields_ = [("ptr", c_vp), ("layout", c_i32), ("cols", c_i32), ("rows", c_i64),
                ("has_ones", c_i32), ("last_rows", c_i32), ("ld", c_i64), ("L", c_i64),
                ("sB", c_i64)] + [(f, c_i32) for f in
                                  ("C", "H", "W", "kh", "kw", "sh", "sw", "ph", "pw", "Ho", "Wo",
                                   "reserved1")]


class FactorJob(ctypes.Structure):
    _fields_ = [("x", Operand), ("alpha", c_f32), ("beta", c_f32), ("F", c_vp), ("ldF", c_i64),
                ("acc", c_vp), ("acc_splits", c_i32), ("acc_beta", c_f32),
                ("seg_ptrs", c_vp), ("nseg", c_i32), ("acc_stride", c_i32)]


class InvertJob(ctypes.Structure):
    _fields_ = [("F", c_vp), ("ldF", c_i64), ("n", c_i32), ("out_kind", c_i32),
                ("scale", c_f64), ("shift", c_f64), ("out", c_vp), ("ldo", c_i64)]


class EigJob(ctypes.Structure):
    _fields_ = [("F", c_vp), ("ldF", c_i64), ("n", c_i32), ("reserved", c_i32),
                ("evals", c_vp), ("evecs", c_vp), ("ldv", c_i64)]


class QuadJob(ctypes.Structure):
    _fields_ = [("J", c_vp), ("ldJ", c_i64), ("nA", c_i32), ("nG", c_i32), ("K1", c_vp),
                ("ld1", c_i64), ("K2", c_vp), ("ld2", c_i64), ("lower1", c_i32),
                ("lower2", c_i32), ("v", c_vp)]


class CovJob(ctypes.Structure):
    _fields_ = [("J", c_vp), ("ldJ", c_i64), ("nA", c_i32), ("nG", c_i32), ("K1", c_vp),
                ("ld1", c_i64), ("K2", c_vp), ("ld2", c_i64), ("lower1", c_i32),
                ("lower2", c_i32)]


class CovOuterJob(ctypes.Structure):
    _fields_ = [("a", c_vp), ("lda", c_i64), ("cols", c_i32), ("has_ones", c_i32), ("D", c_vp),
                ("ldD", c_i64), ("nG", c_i32), ("reserved", c_i32), ("K1", c_vp), ("ld1", c_i64),
                ("K2", c_vp), ("ld2", c_i64), ("lower1", c_i32), ("lower2", c_i32)]


class DrawJob(ctypes.Structure):
    _fields_ = [("rows", CovJob), ("Z", c_vp), ("ldZ", c_i64)]


class DrawOuterJob(ctypes.Structure):
    _fields_ = [("rows", CovOuterJob), ("Z", c_vp), ("ldZ", c_i64)]


class CovConvRowsJob(ctypes.Structure):
    _fields_ = [("x", Operand), ("D", c_vp), ("ldD", c_i64), ("nG", c_i32), ("reserved", c_i32),
                ("M", c_vp), ("ldM", c_i64)]


class CovSweepJob(ctypes.Structure):
    _fields_ = [("J", c_vp), ("ldJ", c_i64), ("nA", c_i32), ("nG", c_i32), ("VA", c_vp),
                ("ldA", c_i64), ("VG", c_vp), ("ldG", c_i64), ("wA", c_vp), ("ldwA", c_i64),
                ("wG", c_vp), ("ldwG", c_i64)]


class CovOuterSweepJob(ctypes.Structure):
    _fields_ = [("a", c_vp), ("lda", c_i64), ("cols", c_i32), ("has_ones", c_i32), ("D", c_vp),
                ("ldD", c_i64), ("nG", c_i32), ("reserved", c_i32), ("VA", c_vp), ("ldA", c_i64),
                ("VG", c_vp), ("ldG", c_i64), ("wA", c_vp), ("ldwA", c_i64), ("wG", c_vp),
                ("ldwG", c_i64)]


class CovFullJob(ctypes.Structure):
    _fields_ = [("J", c_vp), ("ldJ", c_i64), ("nA", c_i32), ("nG", c_i32), ("VA", c_vp),
                ("ldA", c_i64), ("VG", c_vp), ("ldG", c_i64), ("W", c_vp), ("ldW", c_i64)]


class CovOuterFullJob(ctypes.Structure):
    _fields_ = [("a", c_vp), ("lda", c_i64), ("cols", c_i32), ("has_ones", c_i32), ("D", c_vp),
                ("ldD", c_i64), ("nG", c_i32), ("reserved", c_i32), ("VA", c_vp), ("ldA", c_i64),
                ("VG", c_vp), ("ldG", c_i64), ("W", c_vp), ("ldW", c_i64)]


class InfCovJob(ctypes.Structure):
    _fields_ = [("J", c_vp), ("ldJ", c_i64), ("nA", c_i32), ("nG", c_i32), ("UA", c_vp),
                ("ldA", c_i64), ("ra", c_i32), ("UG", c_vp), ("ldG", c_i64), ("rg", c_i32),
                ("W", c_vp), ("ldW", c_i64), ("F", c_vp), ("ldF", c_i64)]


class InfCovOuterJob(ctypes.Structure):
    _fields_ = [("a", c_vp), ("lda", c_i64), ("cols", c_i32), ("has_ones", c_i32), ("D", c_vp),
                ("ldD", c_i64), ("nG", c_i32), ("reserved", c_i32), ("UA", c_vp), ("ldA", c_i64),
                ("ra", c_i32), ("UG", c_vp), ("ldG", c_i64), ("rg", c_i32), ("W", c_vp),
                ("ldW", c_i64), ("F", c_vp), ("ldF", c_i64)]


class InfDrawJob(ctypes.Structure):
    _fields_ = [("rows", InfCovJob), ("C", c_vp), ("Binv", c_vp), ("ldB", c_i64), ("Z", c_vp),
                ("ldZ", c_i64), ("E", c_vp), ("ldE", c_i64)]


class InfDrawOuterJob(ctypes.Structure):
    _fields_ = [("rows", InfCovOuterJob), ("C", c_vp), ("Binv", c_vp), ("ldB", c_i64), ("Z", c_vp),
                ("ldZ", c_i64), ("E", c_vp), ("ldE", c_i64)]


class SampleJob(ctypes.Structure):
    _fields_ = [("LA", c_vp), ("ldA", c_i64), ("LG", c_vp), ("ldG", c_i64), ("Z", c_vp),
                ("nA", c_i32), ("nG", c_i32), ("W", c_vp), ("ldW", c_i64), ("bias", c_vp),
                ("wcols", c_i32), ("dense", c_i32)]


class EfbJob(ctypes.Structure):
    _fields_ = [("VA", c_vp), ("ldA", c_i64), ("VG", c_vp), ("ldG", c_i64), ("grad", c_vp),
                ("ld_grad", c_i64), ("state", c_vp), ("ld_state", c_i64), ("diag", c_vp),
                ("ld_diag", c_i64), ("nA", c_i32), ("nG", c_i32), ("accumulate", c_i32),
                ("scale", c_f32)]


class GramJob(ctypes.Structure):
    _fields_ = [("UA", c_vp), ("ldA", c_i64), ("UG", c_vp), ("ldG", c_i64), ("c", c_vp),
                ("sigma", c_vp), ("out", c_vp), ("ldo", c_i64), ("nA", c_i32), ("nG", c_i32),
                ("la", c_i32), ("lg", c_i32)]


class TriJob(ctypes.Structure):
    _fields_ = [("F", c_vp), ("ldF", c_i64), ("n", c_i32), ("reserved", c_i32), ("offset", c_i64)]


# symbol -> (restype, argtypes); every symbol include/kfac_hip.h declares
SIGNATURES = {
    "kfac_factor_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(FactorJob), ctypes.c_int]),
    "kfac_factor_update": (ctypes.c_int, [ctypes.POINTER(FactorJob), ctypes.c_int, c_vp,
                                          ctypes.c_size_t, c_vp]),
    "kfac_factor_accum_plan": (ctypes.c_int, [ctypes.POINTER(FactorJob), ctypes.c_int,
                                              ctypes.POINTER(c_i32), ctypes.POINTER(ctypes.c_size_t)]),
    "kfac_factor_route": (ctypes.c_int, [ctypes.POINTER(FactorJob), ctypes.c_int, ctypes.POINTER(c_i32)]),
    "kfac_factor_flush": (ctypes.c_int, [ctypes.POINTER(FactorJob), ctypes.c_int, c_vp]),
    "kfac_x3_unit_table": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(c_i32), ctypes.c_int]),
    "kfac_x3_task_decode": (ctypes.c_int, [ctypes.POINTER(c_i32), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.POINTER(c_i32)]),
    "kfac_syrk_linear": (ctypes.c_int, [c_vp, c_i64, c_i64, c_i64, ctypes.c_int, c_f32, c_f32,
                                        c_vp, c_i64, c_vp, ctypes.c_size_t, c_vp]),
    "kfac_syrk_conv": (ctypes.c_int, [c_vp, c_i64] + [ctypes.c_int] * 10 + [c_f32, c_f32, c_vp,
                                                                            c_i64, c_vp,
                                                                            ctypes.c_size_t, c_vp]),
    "kfac_syrk_convgrad": (ctypes.c_int, [c_vp, c_i64, ctypes.c_int, c_i64, c_f32, c_f32, c_vp,
                                          c_i64, c_vp, ctypes.c_size_t, c_vp]),
    "kfac_invert_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(InvertJob), ctypes.c_int]),
    "kfac_invert": (ctypes.c_int, [ctypes.POINTER(InvertJob), ctypes.c_int, c_vp,
                                   ctypes.c_size_t, c_vp, c_vp]),
    "kfac_invert_ex": (ctypes.c_int, [ctypes.POINTER(InvertJob), ctypes.c_int, c_vp,
                                      ctypes.c_size_t, c_vp, c_vp, c_vp]),
    "kfac_damped_inv_chol": (ctypes.c_int, [c_vp, ctypes.c_int, c_i64, c_f64, c_f64, c_vp, c_i64,
                                            c_vp, ctypes.c_size_t, c_vp, c_vp]),
    "kfac_eig_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(EigJob), ctypes.c_int]),
    "kfac_syev": (ctypes.c_int, [ctypes.POINTER(EigJob), ctypes.c_int, c_vp, ctypes.c_size_t,
                                 c_vp, c_vp]),
    "kfac_quadform_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(QuadJob), ctypes.c_int,
                                                        c_i64]),
    "kfac_kron_quadform": (ctypes.c_int, [ctypes.POINTER(QuadJob), ctypes.c_int, c_i64,
                                          ctypes.c_int, c_vp, c_vp, ctypes.c_size_t, c_vp]),
    "kfac_cov_conv_rows": (ctypes.c_int, [ctypes.POINTER(CovConvRowsJob), ctypes.c_int, c_i64, ctypes.c_int,
                                          c_vp]),
    "kfac_softmax_mc": (ctypes.c_int, [c_vp, c_i64, c_vp, c_i64, c_i64, c_i64, ctypes.c_int, ctypes.c_int,
                                       c_vp, c_vp, c_vp]),
    "kfac_sample_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(SampleJob), ctypes.c_int]),
    "kfac_sample": (ctypes.c_int, [ctypes.POINTER(SampleJob), ctypes.c_int, ctypes.c_int, c_vp,
                                   ctypes.c_size_t, c_vp]),
    "kfac_efb_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(EfbJob), ctypes.c_int]),
    "kfac_efb_update": (ctypes.c_int, [ctypes.POINTER(EfbJob), ctypes.c_int, c_vp, ctypes.c_size_t,
                                       c_vp]),
    "kfac_gram_workspace_bytes": (ctypes.c_size_t, [ctypes.POINTER(GramJob), ctypes.c_int]),
    "kfac_kron_gram": (ctypes.c_int, [ctypes.POINTER(GramJob), ctypes.c_int, c_vp, ctypes.c_size_t,
                                      c_vp]),
    "kfac_tri_pack": (ctypes.c_int, [ctypes.POINTER(TriJob), ctypes.c_int, c_vp, c_vp]),
    "kfac_tri_unpack": (ctypes.c_int, [ctypes.POINTER(TriJob), ctypes.c_int, c_vp, ctypes.c_int, c_vp]),
    "kfac_profile_enable": (ctypes.c_int, [ctypes.c_int]),
    "kfac_profile_read": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_int64)]),
    "kfac_profile_read_work": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double),
                                              ctypes.POINTER(ctypes.c_double)]),
    "kfac_profile_reset": (ctypes.c_int, []),
    "kfac_set_knob": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "kfac_get_knob": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]),
    "kfac_release": (ctypes.c_int, []),
    "kfac_invert_pipelined": (ctypes.c_int, [ctypes.POINTER(InvertJob), ctypes.c_int, c_vp, ctypes.c_size_t,
                                             c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "kfac_event_create": (ctypes.c_int, [ctypes.POINTER(c_vp)]),
    "kfac_event_create_ex": (ctypes.c_int, [ctypes.POINTER(c_vp), ctypes.c_int]),
    "kfac_event_destroy": (ctypes.c_int, [c_vp]),
    "kfac_event_record": (ctypes.c_int, [c_vp, c_vp]),
    "kfac_stream_wait_event": (ctypes.c_int, [c_vp, c_vp]),
    "kfac_event_query": (ctypes.c_int, [c_vp]),
    "kfac_event_synchronize": (ctypes.c_int, [c_vp]),
    "kfac_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "kfac_version": (ctypes.c_char_p, []),
}
# The job-array covariance and draw calls, each described once: (name, job struct, family, doc).
# Every call is kfac_<name>(jobs, njobs, nb, nc, <family arguments>) with a workspace query
# kfac_<name>_workspace_bytes(jobs, njobs, nb, nc[, nt | ns]); the SIGNATURES entries are made from
# this table here, the module-level wrappers <name> and <name>_workspace_bytes further down.
JOB_CALLS = (
    ("kron_cov", CovJob, "blocks", "kfac_kron_cov: out (nb, nc, nc) (+)= sum_j T_j T_j^T, <= 8 jobs per call."),
    ("kron_cov_outer", CovOuterJob, "blocks",
     "kfac_kron_cov_outer: out (nb, nc, nc) (+)= sum_j s_j V_j V_j^T, <= 8 jobs per call."),
    ("kron_cov_joint", CovJob, "joint",
     """kfac_kron_cov_joint: out (nb*nc, >= nb*nc) with unit column stride (+)= sum_j T_j T_j^T
    over ALL rows of the call, <= 8 jobs per call."""),
    ("kron_cov_outer_joint", CovOuterJob, "joint",
     """kfac_kron_cov_outer_joint: out (nb*nc, >= nb*nc) (+)= sum_j S_j[b, b'] W_j[r, r'], <= 8 jobs
    per call."""),
    ("kron_cov_tiled", CovJob, "tiled",
     """kfac_kron_cov_tiled: out (nb, nc, nc) (+)= sum_j T_j T_j^T per sample, any nc, <= 8 jobs
    per call."""),
    ("kron_cov_outer_tiled", CovOuterJob, "tiled",
     """kfac_kron_cov_outer_tiled: out (nb, nc, nc) (+)= sum_j s_j V_j V_j^T per sample, any nc,
    <= 8 jobs per call."""),
    ("glm_draws", DrawJob, "draws",
     """kfac_glm_draws: out (ns, >= nb*nc) with unit column stride (+)= sum_j Z_j T_j^T, <= 8 jobs
    per call."""),
    ("glm_draws_outer", DrawOuterJob, "draws",
     "kfac_glm_draws_outer: out (ns, >= nb*nc) (+)= sum_j u_b^T Z_{j,s} v_r, <= 8 jobs per call."),
    ("inf_draws", InfDrawJob, "draws",
     """kfac_inf_draws: out (ns, >= nb*nc) with unit column stride (+)= sum_j [ Z_j (C_j o J_j)^T -
    Q_j Y_j^T ], the INF posterior's logit draws from Jacobian rows, <= 8 jobs per call."""),
    ("inf_draws_outer", InfDrawOuterJob, "draws",
     """kfac_inf_draws_outer: out (ns, >= nb*nc) (+)= sum_j [ abar_b^T (C_j o Z_{j,s}) delta_r -
    < y_{j,r}, q_{j,s} > ], Linear layers without their Jacobian rows, <= 8 jobs per call."""),
    ("kron_cov_sweep", CovSweepJob, "weighted",
     "kfac_kron_cov_sweep: out (nt, nb, nc, nc) (+)= the weighted Grams, <= 8 jobs, nt <= 64."),
    ("kron_cov_outer_sweep", CovOuterSweepJob, "weighted",
     "kfac_kron_cov_outer_sweep: out (nt, nb, nc, nc) (+)= the weighted sums, <= 8 jobs, nt <= 64."),
    ("kron_cov_full", CovFullJob, "weighted",
     "kfac_kron_cov_full: out (nt, nb, nc, nc) (+)= the per-entry weighted Grams, <= 8 jobs, nt <= 64."),
    ("kron_cov_outer_full", CovOuterFullJob, "weighted",
     """kfac_kron_cov_outer_full: out (nt, nb, nc, nc) (+)= Q diag(r) Q^T per grid point, <= 8 jobs,
    nt <= 64."""),
    ("kron_cov_sweep_tiled", CovSweepJob, "weighted",
     "kfac_kron_cov_sweep_tiled: kron_cov_sweep with nc not capped, <= 8 jobs, nt <= 64."),
    ("kron_cov_outer_sweep_tiled", CovOuterSweepJob, "weighted",
     "kfac_kron_cov_outer_sweep_tiled: kron_cov_outer_sweep with nc not capped, <= 8 jobs, nt <= 64."),
    ("kron_cov_full_tiled", CovFullJob, "weighted",
     "kfac_kron_cov_full_tiled: kron_cov_full with nc not capped, <= 8 jobs, nt <= 64."),
    ("kron_cov_outer_full_tiled", CovOuterFullJob, "weighted",
     "kfac_kron_cov_outer_full_tiled: kron_cov_outer_full with nc not capped, <= 8 jobs, nt <= 64."),
    ("inf_cov", InfCovJob, "blocks",
     "kfac_inf_cov: out (nb, nc, nc) (+)= sum_j [rows' W-weighted Gram - Gram of F t], <= 8 jobs."),
    ("inf_cov_outer", InfCovOuterJob, "blocks",
     """kfac_inf_cov_outer: out (nb, nc, nc) (+)= sum_j [Delta diag(rho) Delta^T - Gram of F t],
    <= 8 jobs."""),
    ("inf_cov_tiled", InfCovJob, "tiled", "kfac_inf_cov_tiled: inf_cov for any nc (64x64 class tiles), <= 8 jobs."),
    ("inf_cov_outer_tiled", InfCovOuterJob, "tiled",
     "kfac_inf_cov_outer_tiled: inf_cov_outer for any nc (64x64 class tiles), <= 8 jobs."),
)
# family -> (the size argument after nc and its C type, whether `out` is followed by its leading
# dimension ldo); "tiled" is "blocks" in C, the wrappers of the two differ (_blocks_out)
JOB_CALL_FAMILIES = {"blocks": (None, False), "tiled": (None, False), "weighted": (("nt", ctypes.c_int), False),
                     "joint": (None, True), "draws": (("ns", c_i64), True)}
for _name, _job, _family, _ in JOB_CALLS:
    _size, _ldo = JOB_CALL_FAMILIES[_family]
    _head = [ctypes.POINTER(_job), ctypes.c_int, c_i64, ctypes.c_int] + ([_size[1]] if _size else [])
    SIGNATURES[f"kfac_{_name}_workspace_bytes"] = (ctypes.c_size_t, _head)
    SIGNATURES[f"kfac_{_name}"] = (ctypes.c_int, _head + [ctypes.c_int, c_vp] + ([c_i64] if _ldo else []) +
                                   [c_vp, ctypes.c_size_t, c_vp])

# C struct name (include/kfac_hip.h) -> its ctypes mirror, every ctypes.Structure above
STRUCTS = {"kfac_operand": Operand, "kfac_factor_job": FactorJob, "kfac_invert_job": InvertJob,
           "kfac_eig_job": EigJob, "kfac_quad_job": QuadJob, "kfac_cov_job": CovJob,
           "kfac_cov_outer_job": CovOuterJob, "kfac_draw_job": DrawJob, "kfac_draw_outer_job": DrawOuterJob,
           "kfac_cov_conv_rows_job": CovConvRowsJob, "kfac_cov_sweep_job": CovSweepJob,
           "kfac_cov_outer_sweep_job": CovOuterSweepJob, "kfac_cov_full_job": CovFullJob,
           "kfac_cov_outer_full_job": CovOuterFullJob, "kfac_inf_cov_job": InfCovJob,
           "kfac_inf_cov_outer_job": InfCovOuterJob, "kfac_inf_draw_job": InfDrawJob,
           "kfac_inf_draw_outer_job": InfDrawOuterJob, "kfac_sample_job": SampleJob, "kfac_efb_job": EfbJob,
           "kfac_gram_job": GramJob, "kfac_tri_job": TriJob}

_lib = None
_lock = threading.Lock()


class NativeError(RuntimeError):
    pass


def lib():
    """Load libkfac_hip.so (after torch, so the process shares torch's HIP runtime)."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise NativeError(
                        f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                        f"g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
                handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(handle, name)
                    fn.restype = res
                    fn.argtypes = args
                _lib = handle
                # the library's cached hipGraphs / events go while the HIP runtime is
                # still up (Python's atexit runs before the C runtime's exit handlers)
                atexit.register(_release_at_exit)
    return _lib


def _release_at_exit():
    try:
        if _lib is not None and torch.cuda.is_initialized():
            for h in list(_raw_events):
                _lib.kfac_event_destroy(h)
            _raw_events.clear()
            _lib.kfac_release()
    except Exception:  # exiting anyway: never mask the process's own status
        pass


_raw_events = set()  # handles of the live RawEvents (what is left is destroyed at exit)


class RawEvent:
    """A HIP event owned through the C ABI (kfac_event_*): record / wait / query /
    synchronize are one ctypes call each, where torch.cuda.Event and Stream objects
    cost the caller's thread 5-10 us per call.  Created on `device` (default: the
    current HIP device), like torch.cuda.Event on its stream's device; destroyed by
    close() or when the last reference goes (the KFAC event pools hold them)."""
    __slots__ = ("handle", "ordering")

    def __init__(self, device=None, ordering=False):
        """`ordering`: the event only orders one stream after another on the device
        (kfac_event_create_ex flag 1: no system-scope fence); the host must not rely
        on it to see device writes after synchronize()."""
        h = ctypes.c_void_p()
        flags = 1 if ordering else 0
        if device is not None and torch.device(device).index is not None:
            with torch.cuda.device(device):
                check(lib().kfac_event_create_ex(ctypes.byref(h), flags), "kfac_event_create_ex")
        else:
            check(lib().kfac_event_create_ex(ctypes.byref(h), flags), "kfac_event_create_ex")
        self.handle = h.value
        self.ordering = ordering
        _raw_events.add(self.handle)

    def close(self):
        h, self.handle = self.handle, None
        if h is not None and h in _raw_events:
            _raw_events.discard(h)
            _lib.kfac_event_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter shutdown: _release_at_exit owns what is left)
            pass

    def record(self, stream: int):
        check(_lib.kfac_event_record(self.handle, stream), "kfac_event_record")

    def wait_on(self, stream: int):
        """Order `stream`'s later work after this event's recorded work."""
        check(_lib.kfac_stream_wait_event(stream, self.handle), "kfac_stream_wait_event")

    def query(self) -> bool:
        r = _lib.kfac_event_query(self.handle)
        if r < 0:
            check(r, "kfac_event_query")
        return r == 1

    def synchronize(self):
        check(_lib.kfac_event_synchronize(self.handle), "kfac_event_synchronize")


def check(rc: int, what: str):
    if rc != KFAC_OK:
        msg = lib().kfac_strerror(rc).decode()
        raise NativeError(f"{what} failed: {msg} ({rc})")


def require_device(t: torch.Tensor, what: str, owner=None):
    """HIP device + fp32, or raise (no CPU fallback).  `owner` (e.g. the layer) is
    only formatted into the message on failure: this runs on every update."""
    if t.is_cuda and t.dtype == torch.float32:
        return
    where = f"{what} of {owner}" if owner is not None else what
    if not t.is_cuda:
        raise NativeError(f"bnn_kfac_amd runs on the MI355X only: {where} is on {t.device} "
                          f"(no CPU fallback; move the model/tensors to a HIP device)")
    raise TypeError(f"{where}: expected float32 (the reference computes in fp32), got {t.dtype}")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_handle(device: torch.device) -> int:
    """hipStream_t of torch's current stream on `device` (the raw query avoids
    building a Stream object per call)."""
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


class _Workspace:
    """Grow-only device scratch per (device, stream); stream order makes reuse safe."""

    def __init__(self):
        self._bufs = {}

    def get(self, device: torch.device, nbytes: int, stream: int = None, stream_obj=None) -> torch.Tensor:
        """`stream_obj`: the torch stream the work runs on when it is not the current one
        -- a (re)allocation is then made on it, so the caching allocator orders a grown
        buffer's release after that stream's queued work, not the current stream's."""
        key = (device.index, stream_handle(device) if stream is None else stream)
        buf = self._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            if stream_obj is not None:
                with torch.cuda.stream(stream_obj):
                    buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            else:
                buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self._bufs[key] = buf
        return buf


workspace = _Workspace()
_info_bufs = {}  # (device, stream, jobs) -> the device verdict vector of kfac_invert


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def as_array(ctype, items):
    return (ctype * len(items))(*items)


# ------------------------------------------------------------------ op wrappers
def factor_update(jobs, device: torch.device):
    if not jobs:
        return
    L = lib()
    arr = as_array(FactorJob, jobs)
    need = L.kfac_factor_workspace_bytes(arr, len(jobs))
    stream = stream_handle(device)
    ws = workspace.get(device, need, stream)
    rc = L.kfac_factor_update(arr, len(jobs), ws.data_ptr(), ws.numel(), stream)
    if rc != KFAC_OK:
        check(rc, "kfac_factor_update")


def factor_accum_plan(jobs):
    """[(splits, bytes)] of each job's deferred-reduction accumulator."""
    arr = as_array(FactorJob, jobs)
    splits = (c_i32 * len(jobs))()
    nbytes = (ctypes.c_size_t * len(jobs))()
    check(lib().kfac_factor_accum_plan(arr, len(jobs), splits, nbytes), "kfac_factor_accum_plan")
    return list(zip(splits, nbytes))


def factor_route(jobs):
    """[kfac_prof_id] of the kernel family each job's launch group is first routed to
    (kfac_factor_route: host only, no device call)."""
    family = (c_i32 * len(jobs))()
    check(lib().kfac_factor_route(as_array(FactorJob, jobs), len(jobs), family), "kfac_factor_route")
    return list(family)


def factor_flush(jobs, device: torch.device, stream: int = None):
    """kfac_factor_flush on torch's current stream, or on the raw HIP stream `stream`."""
    if jobs:
        check(lib().kfac_factor_flush(as_array(FactorJob, jobs), len(jobs),
                                      stream_handle(device) if stream is None else stream),
              "kfac_factor_flush")


def invert(jobs, device: torch.device, inputs_read=None) -> torch.Tensor:
    """Launch the grouped inversion on torch's current stream; returns the DEVICE info
    tensor (int32, one per job).  `inputs_read` (a torch.cuda.Event, optional) is
    recorded right after the launches that read the factors (kfac_invert_ex)."""
    L = lib()
    arr = as_array(InvertJob, jobs)
    need = L.kfac_invert_workspace_bytes(arr, len(jobs))
    stream = stream_handle(device)
    ws = workspace.get(device, need, stream)
    # a fresh verdict tensor per call (zeroed by kfac_invert): callers may hold several
    # calls' verdicts at once (the pooled buffer is only invert_pipelined's, whose
    # verdict is copied to host on the same stream before the buffer is written again)
    info = torch.empty(len(jobs), dtype=torch.int32, device=device)
    ev = None
    if inputs_read is not None:
        ev = inputs_read.cuda_event
    check(L.kfac_invert_ex(arr, len(jobs), ws.data_ptr(), ws.numel(), info.data_ptr(), ev, stream),
          "kfac_invert_ex")
    return info


def invert_pipelined(jobs, device: torch.device, info_host: torch.Tensor, order: "RawEvent",
                     inputs_read, done: "RawEvent", main: int, side: int, side_stream=None) -> torch.Tensor:
    """kfac_invert_pipelined: `side` ordered after `main`, the grouped inversion on `side`
    (`inputs_read` recorded after the F-reading launch), the verdict copied into the
    pinned `info_host`, `done` recorded on `side`.  Returns the device verdict vector:
    a buffer pooled per (device, side stream, job count) that the next such call on
    that stream overwrites -- read `info_host` (after `done`), or clone it first."""
    L = lib()
    arr = as_array(InvertJob, jobs)
    need = L.kfac_invert_workspace_bytes(arr, len(jobs))
    ws = workspace.get(device, need, side, side_stream)
    key = (device.index, side, len(jobs))
    info = _info_bufs.get(key)
    if info is None:
        info = _info_bufs[key] = torch.empty(len(jobs), dtype=torch.int32, device=device)
    check(L.kfac_invert_pipelined(arr, len(jobs), ws.data_ptr(), ws.numel(), info.data_ptr(),
                                  info_host.data_ptr(), order.handle,
                                  inputs_read.handle if inputs_read is not None else None,
                                  done.handle, main, side), "kfac_invert_pipelined")
    return info


def tri_jobs(factors):
    """[TriJob] of square row-major factors laid out back to back in a packed
    lower-triangle buffer, and that buffer's length (elements)."""
    jobs, off = [], 0
    for F in factors:
        n = F.shape[0]
        if F.dim() != 2 or F.shape[1] != n or F.stride(1) != 1:
            raise NativeError(f"tri pack: factor must be square with unit column stride, got "
                              f"{tuple(F.shape)} / {F.stride()}")
        jobs.append(TriJob(F.data_ptr(), F.stride(0), n, 0, off))
        off += n * (n + 1) // 2
    return jobs, off


def tri_pack(jobs, packed: torch.Tensor) -> None:
    """kfac_tri_pack on torch's current stream of packed's device."""
    check(lib().kfac_tri_pack(as_array(TriJob, jobs), len(jobs), packed.data_ptr(),
                              stream_handle(packed.device)), "kfac_tri_pack")


def tri_unpack(jobs, packed: torch.Tensor, mode: int) -> None:
    """kfac_tri_unpack (TRI_SYMMETRIC mirrors, TRI_LOWER zeroes the upper triangle)."""
    check(lib().kfac_tri_unpack(as_array(TriJob, jobs), len(jobs), packed.data_ptr(), int(mode),
                                stream_handle(packed.device)), "kfac_tri_unpack")


def syev(jobs, device: torch.device) -> torch.Tensor:
    L = lib()
    arr = as_array(EigJob, jobs)
    need = L.kfac_eig_workspace_bytes(arr, len(jobs))
    ws = workspace.get(device, need)
    info = torch.zeros(len(jobs), dtype=torch.int32, device=device)
    check(L.kfac_syev(arr, len(jobs), ptr(ws), ws.numel(), ptr(info), stream_handle(device)),
          "kfac_syev")
    return info


def kron_quadform(jobs, nb: int, abs_sum: bool, out: torch.Tensor):
    L = lib()
    arr = as_array(QuadJob, jobs)
    need = L.kfac_quadform_workspace_bytes(arr, len(jobs), nb)
    ws = workspace.get(out.device, need)
    check(L.kfac_kron_quadform(arr, len(jobs), nb, int(abs_sum), ptr(out), ptr(ws), ws.numel(),
                               stream_handle(out.device)), "kfac_kron_quadform")


def cov_conv_rows_job(x: Operand, D: torch.Tensor, ldD: int, nG: int, M: torch.Tensor, ldM: int) -> CovConvRowsJob:
    """One Conv2d layer of kfac_cov_conv_rows: x the PATCH operand of its input (patch_operand),
    D its output Jacobian with rows (b, c) ldD apart, M the rows to write, ldM apart."""
    require_device(D, "D")
    require_device(M, "M")
    return CovConvRowsJob(x, D.data_ptr(), ldD, nG, 0, M.data_ptr(), ldM)


def cov_conv_rows(jobs, nb: int, nc: int, device: torch.device = None) -> None:
    """kfac_cov_conv_rows on torch's current stream of `device` (default: the current
    device): Conv2d Jacobian rows M[b, c] = unfold(a_b) D[b, c]^T, <= 8 jobs per call."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    check(lib().kfac_cov_conv_rows(as_array(CovConvRowsJob, jobs), len(jobs), nb, nc,
                                   stream_handle(device)), "kfac_cov_conv_rows")


def _joint_out(out: torch.Tensor, nb: int, nc: int, what: str):
    """The joint calls write nb*nc rows of nb*nc floats, out.stride(0) apart: refuse a view
    they would write outside of."""
    R = nb * nc
    if out.dim() != 2 or out.shape[0] < R or out.shape[1] < R or out.stride(1) != 1 or out.stride(0) < R:
        raise ValueError(f"{what}: out must be 2-D, at least ({R}, {R}), with unit column stride, got "
                         f"{tuple(out.shape)} / {out.stride()}")
    require_device(out, what)


def _blocks_out(out: torch.Tensor, nb: int, nc: int, what: str):
    """The tiled calls write nb contiguous nc x nc blocks: refuse anything else."""
    if tuple(out.shape) != (nb, nc, nc) or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous ({nb}, {nc}, {nc}) tensor, got "
                         f"{tuple(out.shape)} / {out.stride()}")
    require_device(out, what)


def _draws_out(out: torch.Tensor, nb: int, nc: int, ns: int, what: str):
    """The draw calls write ns rows of nb*nc floats, out.stride(0) apart: refuse a view they
    would write outside of."""
    R = nb * nc
    if out.dim() != 2 or out.shape[0] < ns or out.shape[1] < R or out.stride(1) != 1 or \
            (ns > 1 and out.stride(0) < R):
        raise ValueError(f"{what}: out must be 2-D, at least ({ns}, {R}), with unit column stride, got "
                         f"{tuple(out.shape)} / {out.stride()}")
    require_device(out, what)


def _job_call(name: str, struct, family: str, doc: str):
    """(workspace query, call) of one JOB_CALLS row: the jobs as a C array, the query, the scratch
    from the pool, then kfac_<name> on torch's current stream of out's device."""
    symbol, query_symbol = "kfac_" + name, "kfac_" + name + "_workspace_bytes"
    out_check = {"tiled": _blocks_out, "joint": _joint_out, "draws": _draws_out}.get(family)

    def query(jobs, *sizes) -> int:
        return getattr(lib(), query_symbol)(as_array(struct, jobs), len(jobs), *sizes)

    def run(jobs, sizes, out, accumulate):
        if out_check is not None:
            out_check(out, *sizes, name)
        L = lib()
        arr = as_array(struct, jobs)
        ws = workspace.get(out.device, getattr(L, query_symbol)(arr, len(jobs), *sizes))
        ldo = ()
        if family == "joint":
            ldo = (out.stride(0),)
        elif family == "draws":
            ldo = (max(out.stride(0), sizes[0] * sizes[1]),)
        check(getattr(L, symbol)(arr, len(jobs), *sizes, int(accumulate), ptr(out), *ldo, ptr(ws), ws.numel(),
                                 stream_handle(out.device)), symbol)

    # the public signatures, spelled out: (jobs, nb, nc[, nt | ns], out, accumulate=False)
    if family == "weighted":
        def workspace_bytes(jobs, nb: int, nc: int, nt: int) -> int:
            return query(jobs, nb, nc, nt)

        def call(jobs, nb: int, nc: int, nt: int, out: torch.Tensor, accumulate: bool = False):
            run(jobs, (nb, nc, nt), out, accumulate)
    elif family == "draws":
        def workspace_bytes(jobs, nb: int, nc: int, ns: int) -> int:
            return query(jobs, nb, nc, ns)

        def call(jobs, nb: int, nc: int, ns: int, out: torch.Tensor, accumulate: bool = False):
            run(jobs, (nb, nc, ns), out, accumulate)
    else:
        def workspace_bytes(jobs, nb: int, nc: int) -> int:
            return query(jobs, nb, nc)

        def call(jobs, nb: int, nc: int, out: torch.Tensor, accumulate: bool = False):
            run(jobs, (nb, nc), out, accumulate)
    call.__name__ = call.__qualname__ = name
    workspace_bytes.__name__ = workspace_bytes.__qualname__ = name + "_workspace_bytes"
    call.__doc__ = doc
    return workspace_bytes, call


# kron_cov, kron_cov_workspace_bytes, ... inf_cov_outer_tiled, inf_cov_outer_tiled_workspace_bytes
for _row in JOB_CALLS:
    globals()[_row[0] + "_workspace_bytes"], globals()[_row[0]] = _job_call(*_row)


def softmax_mc(mean: torch.Tensor, draws: torch.Tensor, psum: torch.Tensor, hsum: torch.Tensor,
               accumulate: bool = False):
    """kfac_softmax_mc: psum (nb, nc) and hsum (nb,) fp64 (+)= the sums over the ns draws of
    softmax(mean + draws[s]) and of its entropy.  mean (nb, nc) and draws (ns, nb, nc) fp32 with
    unit innermost stride; draws[s] is one contiguous block, the draws draws.stride(0) apart."""
    require_device(mean, "mean")
    require_device(draws, "draws")
    if mean.dim() != 2 or draws.dim() != 3 or tuple(draws.shape[1:]) != tuple(mean.shape):
        raise ValueError(f"mean {tuple(mean.shape)} / draws {tuple(draws.shape)}: expected (nb, nc) and "
                         f"(ns, nb, nc)")
    ns, nb, nc = draws.shape
    if mean.stride(1) != 1 or (nb > 1 and mean.stride(0) < nc):
        mean = mean.contiguous()
    if not draws[0].is_contiguous() or (ns > 1 and draws.stride(0) < nb * nc):
        draws = draws.contiguous()
    for t, shape, what in ((psum, (nb, nc), "psum"), (hsum, (nb,), "hsum")):
        if not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}: expected a contiguous float64 {shape} tensor on the device, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
    check(lib().kfac_softmax_mc(ptr(mean), mean.stride(0) if nb > 1 else nc, ptr(draws),
                                draws.stride(0) if ns > 1 else nb * nc, ns, nb, nc, int(accumulate),
                                ptr(psum), ptr(hsum), stream_handle(mean.device)), "kfac_softmax_mc")


def sample(jobs, device: torch.device, accumulate: bool) -> None:
    """kfac_sample, <= 8 jobs per launch pair (KFAC.sample / sample_and_replace)."""
    L = lib()
    for i in range(0, len(jobs), 8):
        chunk = jobs[i:i + 8]
        arr = as_array(SampleJob, chunk)
        ws = workspace.get(device, L.kfac_sample_workspace_bytes(arr, len(chunk)))
        check(L.kfac_sample(arr, len(chunk), int(accumulate), ptr(ws), ws.numel(),
                            stream_handle(device)), "kfac_sample")


def efb_update(jobs, device: torch.device) -> None:
    """kfac_efb_update, <= 8 layers per launch pair (EFB.update)."""
    L = lib()
    for i in range(0, len(jobs), 8):
        chunk = jobs[i:i + 8]
        arr = as_array(EfbJob, chunk)
        ws = workspace.get(device, L.kfac_efb_workspace_bytes(arr, len(chunk)))
        check(L.kfac_efb_update(arr, len(chunk), ptr(ws), ws.numel(), stream_handle(device)),
              "kfac_efb_update")


def efb_job(VA: torch.Tensor, VG: torch.Tensor, grad: torch.Tensor, state: torch.Tensor,
            diag, accumulate: bool, scale: float) -> EfbJob:
    """One layer of EFB.update: state (+)= (VG^T grad VA)^2, diag (+)= grad^2 * scale."""
    nG, nA = grad.shape
    for t, what in ((VA, "V_A"), (VG, "V_G"), (grad, "grad"), (state, "state")):
        require_device(t, what)
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: expected a 2-D tensor with unit column stride")
    if tuple(VA.shape) != (nA, nA) or tuple(VG.shape) != (nG, nG) or tuple(state.shape) != (nG, nA):
        raise ValueError(f"EFB shapes: V_A {tuple(VA.shape)}, V_G {tuple(VG.shape)}, grad "
                         f"{tuple(grad.shape)}, state {tuple(state.shape)}")
    j = EfbJob()
    j.VA, j.ldA, j.VG, j.ldG = VA.data_ptr(), VA.stride(0), VG.data_ptr(), VG.stride(0)
    j.grad, j.ld_grad = grad.data_ptr(), grad.stride(0)
    j.state, j.ld_state = state.data_ptr(), state.stride(0)
    if diag is not None:
        require_device(diag, "diag")
        if tuple(diag.shape) != (nG, nA) or diag.stride(1) != 1:
            raise ValueError(f"diag: expected ({nG}, {nA}) row-major, got {tuple(diag.shape)}")
        j.diag, j.ld_diag = diag.data_ptr(), diag.stride(0)
    j.nA, j.nG, j.accumulate, j.scale = nA, nG, int(accumulate), float(scale)
    return j


def kron_gram(UA: torch.Tensor, UG: torch.Tensor, c: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """kfac_kron_gram: (la*lg)^2 = diag(sigma) V^T V diag(sigma), V = c * kron(UA, UG)
    (INF.pre_sampler, curvatures.py:548-580), never forming V."""
    for t, what in ((UA, "U_A"), (UG, "U_G"), (c, "correction"), (sigma, "sigma")):
        require_device(t, what)
    UA = UA if UA.stride(1) == 1 else UA.contiguous()
    UG = UG if UG.stride(1) == 1 else UG.contiguous()
    c, sigma = c.contiguous(), sigma.contiguous()
    nA, la = UA.shape
    nG, lg = UG.shape
    if c.numel() != nA * nG or sigma.numel() != la * lg:
        raise ValueError(f"kron_gram: c has {c.numel()} (want {nA * nG}), sigma {sigma.numel()} "
                         f"(want {la * lg}) elements")
    out = torch.empty(la * lg, la * lg, device=UA.device, dtype=torch.float32)
    j = GramJob()
    j.UA, j.ldA, j.UG, j.ldG = UA.data_ptr(), UA.stride(0), UG.data_ptr(), UG.stride(0)
    j.c, j.sigma, j.out, j.ldo = c.data_ptr(), sigma.data_ptr(), out.data_ptr(), out.stride(0)
    j.nA, j.nG, j.la, j.lg = nA, nG, la, lg
    L = lib()
    arr = as_array(GramJob, [j])
    ws = workspace.get(UA.device, L.kfac_gram_workspace_bytes(arr, 1))
    check(L.kfac_kron_gram(arr, 1, ptr(ws), ws.numel(), stream_handle(UA.device)), "kfac_kron_gram")
    return out


def sample_job(LA: torch.Tensor, LG: torch.Tensor, z: torch.Tensor, W: torch.Tensor, wcols: int,
               bias: torch.Tensor = None, dense: bool = False) -> SampleJob:
    """(LA z LG^T)^T into W (nG rows, columns < wcols) and, when wcols == nA - 1, its
    last column into bias."""
    for t in (LA, LG, z, W) + ((bias,) if bias is not None else ()):
        require_device(t, "sample operand")
        if t.stride(-1) != 1:
            raise NativeError("sample operands need a unit column stride")
    nA, nG = LA.shape[0], LG.shape[0]
    if tuple(z.shape) != (nA, nG) or not z.is_contiguous():
        raise NativeError(f"sample: z must be a contiguous ({nA}, {nG}) tensor")
    if W.dim() != 2 or W.shape[0] != nG or W.shape[1] < wcols:
        raise NativeError(f"sample: output must be ({nG}, >= {wcols})")
    return SampleJob(LA.data_ptr(), LA.stride(0), LG.data_ptr(), LG.stride(0), z.data_ptr(), nA, nG,
                     W.data_ptr(), W.stride(0), bias.data_ptr() if bias is not None else None,
                     wcols, int(dense))


# ---------------------------------------------------------------- job builders
def rowmajor_operand(x: torch.Tensor, has_ones: bool) -> Operand:
    """(rows, cols) row-major matrix, unit column stride (Linear a / g_rec)."""
    rows, cols = x.shape
    ld, unit = x.stride()
    assert unit == 1
    # positional constructor: one ctypes call instead of an attribute write per field
    return Operand(x.data_ptr(), ROWMAJOR, cols, rows, int(has_ones), 0, max(ld, cols))


def channel_operand(g: torch.Tensor) -> Operand:
    """Conv2d output gradient (B, C, Ho, Wo) contiguous: rows = B*Ho*Wo, cols = C."""
    assert g.dim() == 4 and g.is_contiguous()
    B, C, Ho, Wo = g.shape
    op = Operand()
    op.ptr, op.layout, op.cols = g.data_ptr(), CHANNEL, C
    op.L = Ho * Wo
    op.sB = C * Ho * Wo
    op.rows = B * Ho * Wo
    return op


def patch_operand(x: torch.Tensor, kernel, padding, stride, has_ones: bool) -> Operand:
    """Implicit F.unfold(x, kernel, padding=, stride=) of a contiguous (B,C,H,W) input."""
    assert x.dim() == 4 and x.is_contiguous()
    B, C, H, W = x.shape
    kh, kw = kernel
    ph, pw = padding
    sh, sw = stride
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    if Ho <= 0 or Wo <= 0:
        raise RuntimeError(f"unfold: kernel {kernel} with padding {padding} larger than input {H}x{W}")
    op = Operand()
    op.ptr, op.layout = x.data_ptr(), PATCH
    op.C, op.H, op.W, op.kh, op.kw, op.sh, op.sw, op.ph, op.pw, op.Ho, op.Wo = \
        C, H, W, kh, kw, sh, sw, ph, pw, Ho, Wo
    op.L = Ho * Wo
    op.sB = C * H * W
    op.rows = B * Ho * Wo
    op.cols = C * kh * kw
    op.has_ones = int(has_ones)
    return op


def factor_job(op: Operand, F: torch.Tensor, alpha: float, beta: float) -> FactorJob:
    return FactorJob(op, alpha, beta, F.data_ptr(), F.stride(0))


def segment_table(ptrs):
    """HOST int64 array of batch base pointers for a multi-batch factor job
    (kfac_factor_job.seg_ptrs).  kfac_factor_update reads it during the call and
    passes the bases to the kernel as launch arguments: no device copy, no sync.
    The caller keeps the returned array alive until the call returns."""
    return (ctypes.c_int64 * len(ptrs))(*ptrs)


def table_ptr(table) -> int:
    return ctypes.addressof(table)


def invert_job(F: torch.Tensor, out: torch.Tensor, scale: float, shift: float,
               kind: int = OUT_INV_CHOL) -> InvertJob:
    # (one positional constructor call: field-by-field assignment costs ~4x the host time)
    return InvertJob(F.data_ptr(), F.stride(0), F.shape[0], kind, scale, shift, out.data_ptr(),
                     out.stride(0))


# ------------------------------------------------------------------ profiling
def profile_enable(on: bool = True):
    check(lib().kfac_profile_enable(int(on)), "kfac_profile_enable")


def profile_reset():
    check(lib().kfac_profile_reset(), "kfac_profile_reset")


def profile_read(kid: int):
    """(total milliseconds, launches) of the library's launches of kernel `kid`
    recorded since the last reset (HIP events on the launch stream)."""
    ms, n = ctypes.c_double(), ctypes.c_int64()
    check(lib().kfac_profile_read(kid, ctypes.byref(ms), ctypes.byref(n)), "kfac_profile_read")
    return ms.value, n.value


def profile_read_work(kid: int):
    """(total milliseconds, launches, algorithmic flops, algorithmic bytes) of slot `kid`
    since the last reset (kfac_profile_read_work: a factor slot's flops are sum K_rows *
    n (n + 1), its bytes every operand read once)."""
    ms, n = ctypes.c_double(), ctypes.c_int64()
    w, b = ctypes.c_double(), ctypes.c_double()
    check(lib().kfac_profile_read_work(kid, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w), ctypes.byref(b)),
          "kfac_profile_read_work")
    return ms.value, n.value, w.value, b.value


# ------------------------------------------------------------------ knobs
def set_knob(name: str, value: int):
    """Change a per-call knob (KFAC_INV_GRAPH, KFAC_INV_LOOKAHEAD, KFAC_EIG_G, KFAC_EIG_RB)
    between calls; the library reads its environment once, at load."""
    check(lib().kfac_set_knob(name.encode(), int(value)), f"kfac_set_knob({name})")


def get_knob(name: str) -> int:
    v = ctypes.c_int()
    check(lib().kfac_get_knob(name.encode(), ctypes.byref(v)), f"kfac_get_knob({name})")
    return v.value
