"""Shapes and the recorded fp32-chain error of the class-tiled INF GLM-predictive tests
(test_gpu_glm_inf_tiled.py, test_glm_inf_tiled_host.py).  Inputs and fp64 references are
glm_inf_cases' own generators (outer_case, dense_case, int_outer_case, int_dense_case), which
take nc; every shape below is the smallest that reaches its edge, and for every one of them
the generators' asserts (the cancellation cap, the integer bound) pass."""
import numpy as np

import glm_inf_cases as C

# (cols, has_ones, nG, ra, rg, nb, nc)
OUTER_SHAPES = [(20, 1, 31, 7, 3, 2, 33),        # first nc past the cap, one tile pair
                (63, 1, 10, 5, 3, 3, 65),        # a second class tile of one row: three pairs
                (12, 1, 70, 2, 66, 2, 100),      # a CIFAR-100 head; rg > 64
                (130, 1, 130, 33, 9, 2, 129),    # three class tiles, six pairs
                (3, 0, 2050, 2, 2, 1, 66),       # term 1's K = nG crosses JSEG = 2048; no bias
                (40, 1, 70, 33, 63, 1, 65)]      # r = 2079 crosses JSEG in term 2
# (nA, nG, ra, rg, nb, nc)
DENSE_SHAPES = [(5, 3, 2, 2, 2, 33),
                (64, 10, 8, 4, 2, 65),
                (33, 65, 5, 7, 2, 100),          # K = 2145 crosses JSEG
                (26, 5, 26, 5, 1, 129),
                (40, 70, 33, 63, 1, 65),         # r = 2079
                (70, 70, 65, 2, 1, 66)]          # ra > 64
# nc <= 32 is valid for the tiled calls (one tile pair): against the capped calls
CAPPED_OUTER = [(63, 1, 10, 5, 3, 3, 10), (20, 1, 31, 7, 31, 2, 32), (300, 0, 257, 3, 2, 3, 4)]
CAPPED_DENSE = [(64, 10, 8, 4, 3, 10), (26, 5, 26, 5, 3, 32), (33, 65, 5, 7, 2, 5)]
# whole-buffer integer-exact cases: keyword arguments of int_outer_case / int_dense_case
INT_OUTER = [dict(nb=2, nc=65), dict(nb=1, nc=129)]
INT_DENSE = [dict(nb=2, nc=65)]                  # K = 33 * 65 = 2145: a second segment

# Tolerance: glm_inf_cases' rule.  rtol = SCALE, atol = SCALE * max|first term|, SCALE =
# max(1e-5, 4 x the fp32 stage chain's error measured on the CPU over the shapes above)
# (fp32_chain_error below; test_glm_inf_tiled_host.py re-measures it and checks this record).
# Never derived from the device's output.
MEASURED_FP32_CHAIN = 6.5e-7  # worst case: dense (70, 70, 65, 2, 1, 66); outer worst 4.6e-7 at (3, 0, 2050, 2, 2, 1, 66)
SCALE = max(1e-5, 4 * MEASURED_FP32_CHAIN)  # = 1e-5: four times the measured error is 2.6e-6
assert SCALE == C.SCALE


def fp32_chain_errors():
    """{("outer" | "dense", shape): |fp32 chain - fp64 reference| / max|first term|}."""
    out = {}
    for shape in OUTER_SHAPES:
        a, D, UA, UG, W, F, ref, top = C.outer_case(*shape)
        out[("outer", shape)] = float(np.abs(C.fp32_outer(a, shape[1], D, UA, UG, W, F) - ref).max() / top)
    for shape in DENSE_SHAPES:
        J, UA, UG, W, F, ref, top = C.dense_case(*shape)
        out[("dense", shape)] = float(np.abs(C.fp32_dense(J, shape[0], shape[1], UA, UG, W, F) - ref).max() / top)
    return out
