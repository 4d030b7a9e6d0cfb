"""Time the class-tiled INF GLM covariance calls (variance.kron_covariance_inf_tiled,
kron_covariance_outer_inf_tiled) on a 512 -> 100 head (nA = 513 with the bias, nG = 100,
nc = 100), nb = 64, ra = rg = 10, on synthetic inputs generated from a seed on the device
(leading columns of orthogonal matrices for UA, UG; weights 10^U(-2, 2); F lower-triangular,
scaled so the second term is about half the first), both routes (the dense route's rows are
outer([a | 1], delta)).  Per route, alternated call by call in one session:
  inf_tiled_ms        : the new call
  full_tiled_ms       : kron_covariance_full_tiled / kron_covariance_outer_full_tiled (nt = 1)
                        at the same shape with square orthogonal VA, VG: the nearest existing
                        call, ONE Gram per tile pair and full-width projections
  inf_capped_nc32_ms / inf_tiled_nc32_ms : the capped INF call and the new one on the first 32
                        outputs of the same inputs
  err_vs_fp64_over_max_first : the new call against the same formula from torch ops in fp64 on
                        the same fp32 inputs, over max|first term| (once, outside the timings)
GPU times are HIP-event times of single calls after a warm-up, medians over `--reps` calls.
There is no pass mark.  Prints one JSON line per route, then the whole."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_glm_full import alternate_ms  # noqa: E402
from bnn_kfac_amd import _native as N  # noqa: E402
from bnn_kfac_amd.variance import (kron_covariance_full_tiled, kron_covariance_inf,  # noqa: E402
                                   kron_covariance_inf_tiled, kron_covariance_outer_full_tiled,
                                   kron_covariance_outer_inf, kron_covariance_outer_inf_tiled)

NB, NC, NA, NG, RA, RG = 64, 100, 513, 100, 10, 10


def fp64_terms(abar, D, UA, UG, W, F):
    """(first, second) of the factored formula in fp64 torch ops."""
    abar, D, UA, UG, W, F = (t.double() for t in (abar, D, UA, UG, W, F))
    rho = (abar * abar) @ W
    H = torch.einsum("ip,bi,ig->bpg", UA, abar, W)
    t = torch.einsum("bpg,bcg,gq->bcpq", H, D, UG).reshape(D.shape[0], D.shape[1], -1)
    y = t @ F.T
    return torch.einsum("bcg,bg,bdg->bcd", D, rho, D), torch.einsum("bcr,bdr->bcd", y, y)


def run_route(route, dev, args):
    gen = torch.Generator(device=dev).manual_seed(1000 * NA + NG)
    rand = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    a, D = rand(NB, NA - 1), rand(NB, NC, NG)
    VA, VG = torch.linalg.qr(rand(NA, NA))[0].contiguous(), torch.linalg.qr(rand(NG, NG))[0].contiguous()
    UA, UG = VA[:, :RA].contiguous(), VG[:, :RG].contiguous()
    W = 10.0 ** (4.0 * torch.rand(NA, NG, device=dev, generator=gen) - 2.0)
    abar = torch.cat([a, a.new_ones(NB, 1)], dim=1)
    F = torch.tril(rand(RA * RG, RA * RG))
    first, second = fp64_terms(abar, D, UA, UG, W, F)
    F = (F * torch.sqrt(0.5 * first.abs().max() / second.abs().max()).float()).contiguous()
    first, second = fp64_terms(abar, D, UA, UG, W, F)
    if route == "dense":
        J = torch.einsum("bi,bcg->bcig", abar, D).reshape(NB, NC, NA * NG).contiguous()
        J32 = J[:, :32].contiguous()
        new = lambda: kron_covariance_inf_tiled([(J, UA, UG, W, F)])  # noqa: E731
        full = lambda: kron_covariance_full_tiled([(J, VA, VG, W)])  # noqa: E731
        capped = lambda: kron_covariance_inf([(J32, UA, UG, W, F)])  # noqa: E731
        new32 = lambda: kron_covariance_inf_tiled([(J32, UA, UG, W, F)])  # noqa: E731
    else:
        D32 = D[:, :32].contiguous()
        new = lambda: kron_covariance_outer_inf_tiled([(a, D, UA, UG, W, F)])  # noqa: E731
        full = lambda: kron_covariance_outer_full_tiled([(a, D, VA, VG, W)])  # noqa: E731
        capped = lambda: kron_covariance_outer_inf([(a, D32, UA, UG, W, F)])  # noqa: E731
        new32 = lambda: kron_covariance_outer_inf_tiled([(a, D32, UA, UG, W, F)])  # noqa: E731
    names = ["inf_tiled_ms", "full_tiled_ms", "inf_capped_nc32_ms", "inf_tiled_nc32_ms"]
    r = dict(zip(names, alternate_ms([new, full, capped, new32], args.warmup, args.reps)))
    r["err_vs_fp64_over_max_first"] = float((new().double() - (first - second)).abs().max() / first.abs().max())
    r["tiled_nc32_vs_capped_over_max_first"] = float(
        (new32().double() - capped().double()).abs().max() / first[:, :32, :32].abs().max())
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--routes", default="outer,dense")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": "class-tiled INF GLM covariance, 512 -> 100 head", "lib": N.LIB_PATH,
           "nA": NA, "nG": NG, "ra": RA, "rg": RG, "nb": NB, "nc": NC}
    for route in args.routes.split(","):
        out[route] = run_route(route, dev, args)
        print(json.dumps({route: out[route]}), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
