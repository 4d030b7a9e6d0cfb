"""Times the class-tiled per-sample covariance (kron_covariance_tiled /
kron_covariance_outer_tiled) against what the library offered for the same blocks before it:
a loop of nb joint calls with nb = 1 each.  Shapes: a 256 -> 100 head at nb = 64 (both
routes) and a 512 -> 1000 head at nb = 16 (outer route).

Each case warms both versions up, checks that they agree (the dense route bitwise), then
alternates them for ROUNDS rounds, each version's round sized to at least WINDOW seconds of
calls (from one timed probe round), a device synchronise around every round.  Prints one
JSON line per case (ms per call: median, min, max over the rounds; the workspace bytes of the
tiled call) and writes them to the file given as argv[1].  Needs a HIP device: there is no
CPU path.  Run from the repository root: PYTHONPATH=. python tools/gpu/time_tiled_cov.py"""
import json
import statistics
import sys
import time

import torch

from bnn_kfac_amd import _native as N
from bnn_kfac_amd import variance as V

ROUNDS, PROBE, WINDOW = 7, 10, 0.25
BUDGET = 1 << 33  # one call over all samples: no chunking in either version


def _factors(g, nA, nG, dev):
    K1 = torch.tril(torch.randn(nA, nA, generator=g, device=dev) / nA ** 0.5)
    K2 = torch.tril(torch.randn(nG, nG, generator=g, device=dev) / nG ** 0.5)
    return K1, K2


def _timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _ab(name, tiled, loop, extra):
    a, b = tiled(), loop()
    torch.cuda.synchronize()
    same = bool(torch.equal(a, b))
    rel = float((a - b).abs().max() / b.abs().max())
    for _ in range(2):
        tiled(), loop()
    na, nb = (max(PROBE, int(WINDOW * 1e3 / _timed(fn, PROBE)) + 1) for fn in (tiled, loop))
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(_timed(tiled, na))
        tb.append(_timed(loop, nb))
    rec = {"case": name, "bitwise_equal": same, "max_rel_diff": rel, "calls_per_round": [na, nb],
           "tiled_ms": {"median": statistics.median(ta), "min": min(ta), "max": max(ta)},
           "joint_loop_ms": {"median": statistics.median(tb), "min": min(tb), "max": max(tb)}}
    rec.update(extra)
    print(json.dumps(rec), flush=True)
    return rec


def dense_case(dev, g, nA, nG, nb, nc):
    K1, K2 = _factors(g, nA, nG, dev)
    J = torch.randn(nb, nc, nA * nG, generator=g, device=dev)
    terms = [(J, K1, K2)]
    jobs = [N.CovJob(*j) for j in V._cov_jobs(terms, True, "time")[1]]
    extra = {"shape": [nA, nG, nb, nc],
             "tiled_workspace_bytes": N.kron_cov_tiled_workspace_bytes(jobs, nb, nc),
             "joint_nb1_workspace_bytes": N.kron_cov_joint_workspace_bytes(jobs, 1, nc)}

    def tiled():
        return V.kron_covariance_tiled(terms, max_workspace_bytes=BUDGET)

    def loop():
        return torch.cat([V.kron_covariance_joint([(J[b:b + 1], K1, K2)], max_workspace_bytes=BUDGET)[:, :, 0]
                          for b in range(nb)])

    return _ab(f"dense {nA - 1}->{nG} nb={nb}", tiled, loop, extra)


def outer_case(dev, g, cols, nG, nb, nc):
    K1, K2 = _factors(g, cols + 1, nG, dev)
    a = torch.randn(nb, cols, generator=g, device=dev)
    D = torch.randn(nb, nc, nG, generator=g, device=dev)
    terms = [(a, D, K1, K2)]
    jobs = [N.CovOuterJob(*j) for j in V._cov_outer_jobs(terms, True, "time")[1]]
    extra = {"shape": [cols, 1, nG, nb, nc],
             "tiled_workspace_bytes": N.kron_cov_outer_tiled_workspace_bytes(jobs, nb, nc),
             "joint_nb1_workspace_bytes": N.kron_cov_outer_joint_workspace_bytes(jobs, 1, nc)}

    def tiled():
        return V.kron_covariance_outer_tiled(terms, max_workspace_bytes=BUDGET)

    def loop():
        return torch.cat([V.kron_covariance_outer_joint([(a[b:b + 1], D[b:b + 1], K1, K2)],
                                                        max_workspace_bytes=BUDGET)[:, :, 0] for b in range(nb)])

    return _ab(f"outer {cols}->{nG} nb={nb}", tiled, loop, extra)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("time_tiled_cov.py needs a HIP device")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    out = [dense_case(dev, g, 257, 100, 64, 100),
           outer_case(dev, g, 256, 100, 64, 100),
           outer_case(dev, g, 512, 1000, 16, 1000)]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
