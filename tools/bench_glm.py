"""Time the GLM predictive (variance.kron_covariance / glm_predictive).

Workloads (random init, KFAC factors accumulated over synthetic batches, inverted at
(0.04, 200)):
  mlp       : the MNIST MLP 784-128-10 (layers 785x128, 129x10), nb = 64, nc = 10
  basenet15k: BaseNet_15k's four layers (26x5, 126x10, 161x80, 81x10), nb = 256, nc = 10
  c5        : the wide MLP 784-4096-4096-10 (layers 785x4096, 4097x4096, 4097x10), nb = 64,
              nc = 10, factored route only (one dense Jacobian row of it is 67 MB)

Per workload, on the same Jacobians and factors:
  cov_ms        : kron_covariance (kfac_kron_cov) alone
  torch_cov_ms  : the same contraction composed from torch ops on the same GPU,
                  T = L_A^T @ M @ L_G, cov = sum_l T.flatten(2) @ T.flatten(2).mT
  cpu_cov_ms    : that composition in fp32 on the host, 16 threads
  glm_ms        : glm_predictive end to end (vmapped Jacobians + kron_covariance)
  torch_glm_ms  : the same Jacobians + the torch composition
The factored route (glm_predictive(jacobians="factored")), the two routes alternated call
by call in one session:
  cov_linear_dense_ms / cov_linear_outer_ms : the Linear layers alone, kron_covariance on
                  their dense rows against kron_covariance_outer on (input, output Jacobian)
  glm_dense_ms / glm_factored_ms : glm_predictive end to end, both ways
  factored_max_diff_over_max : the two end-to-end covariances, max |diff| / max
`--sweep NT` instead times the damping grid (glm_predictive_sweep) on mlp (factored),
basenet15k (dense) and c5 (factored; `--workloads` selects, one JSON line per workload as it
finishes -- C5's eigh() alone takes minutes), for the grid sizes 1, 4, 16 and NT:
  eigh_ms                 : the one-off KFAC.eigh() (cache dropped before every call)
  sweep_ms[nt]            : glm_predictive_sweep over nt dampings, eigenpairs cached
  loop_ms[nt]             : the same grid as a loop of kfac.invert + glm_predictive
  sweep_cov_ms / loop_cov_ms[nt] : the covariance calls alone on fixed Jacobians or
                            captures (the sweep kernel once; the plain kernel nt times)
  marginal_ms_per_damping : (sweep_ms[16] - sweep_ms[1]) / 15, against
  loop_ms_per_damping     : loop_ms[16] / 16
  sweep_max_diff_over_max : the sweep against the loop's covariances, max |diff| / max
all alternated call by call in one session.
`--joint` instead times the joint covariance across the samples (glm_predictive(joint=True))
on mlp and basenet15k (both routes) and c5 (factored only; `--workloads` selects, one JSON
line per workload), per route on the same inputs, alternated call by call:
  joint_ms      : kron_covariance_joint / kron_covariance_outer_joint alone (factored: the
                  Linear layers)
  torch_ms      : the same quantity from torch ops on the same GPU -- dense: T = L_A^T @ M @ L_G
                  flattened to (nb*nc, nA*nG), sum_l T @ T.mT; factored: (U @ U.mT) expanded
                  over the classes times V @ V.mT
  per_sample_ms : kron_covariance / kron_covariance_outer on the same inputs (the block
                  diagonal alone: what the cross blocks cost on top)
  glm_joint_ms  : glm_predictive(joint=True) end to end
  max_diff_vs_torch_over_max : joint call against the torch composition
and for the dense Gram the algorithmic work kept here: gram_flops = sum_l R (R + 1) K_l (the
lower triangle with its diagonal, 2 flops per multiply-add), gram_bytes = sum_l 4 R K_l (T
read once), and what joint_ms makes of them against the 157.3 TF/s fp32-MFMA peak
(gram_tflops_of_call, a lower bound: the call also runs apply and reduce; a kernel trace of
`--joint --only cov` gives kfac_cov_joint_gram's own time).
`--conv-rows` instead times the Conv2d rows of the factored route on basenet15k (nb = 256) and
on LeNet-5 (conv 1->6 with padding 2 and 6->16, 5x5 kernels; nb = 64), nc = 10, on one
layer_io_jacobians capture, alternated call by call:
  rows_device_ms / rows_torch_ms : conv_jacobian_rows_device (kfac_cov_conv_rows) against
                  conv_jacobian_rows (unfold + einsum + cat) for all conv layers, and per layer
                  under conv_layers with the launch's task count
  rows_device_tflops : 2 nA nG L flops per row over rows_device_ms
  glm_factored_device_rows_ms / glm_factored_torch_rows_ms / glm_dense_ms : glm_predictive end
                  to end, factored with either rows (torch's rows: the route before the device
                  rows existed) and dense
GPU times are HIP-event times of single calls after a warm-up, medians over `--reps`
calls.  apply_flops / gram_bytes are the algorithmic work (2 nA^2 nG + 2 nA nG^2 per
row, halved for the skipped triangle; T read once) for a roofline over kernel times
taken in a profiler run of `--only cov`.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bnn_kfac_amd import _native as N  # noqa: E402
from bnn_kfac_amd import variance as V  # noqa: E402
from bnn_kfac_amd.curvatures import KFAC  # noqa: E402
from bnn_kfac_amd.variance import (damping_weights, glm_predictive, glm_predictive_sweep,  # noqa: E402
                                   kron_covariance, kron_covariance_joint, kron_covariance_outer,
                                   kron_covariance_outer_joint, kron_covariance_outer_sweep,
                                   kron_covariance_sweep, layer_io_jacobians, output_jacobians)


def mlp():
    return nn.Sequential(nn.Linear(784, 128), nn.ReLU(), nn.Linear(128, 10)), (784,), 64


def basenet15k():
    return nn.Sequential(nn.Conv2d(1, 5, 5), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(5, 10, 5), nn.ReLU(),
                         nn.MaxPool2d(2), nn.Flatten(), nn.Linear(160, 80), nn.ReLU(),
                         nn.Linear(80, 10)), (1, 28, 28), 256


def c5():
    return nn.Sequential(nn.Linear(784, 4096), nn.ReLU(), nn.Linear(4096, 4096), nn.ReLU(),
                         nn.Linear(4096, 10)), (784,), 64


def alternate_ms(fns, warmup, reps):
    """Medians of HIP-event times of each of `fns`, called in turn `reps` times."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for fn, t in zip(fns, times):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            t.append(a.elapsed_time(b))
    return [statistics.median(t) for t in times]


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def torch_cov(terms):
    cov = 0
    for J, LA, LG in terms:
        nA, nG = LA.shape[0], LG.shape[0]
        T = (LA.T @ J.view(J.shape[0], J.shape[1], nA, nG) @ LG).flatten(2)
        cov = cov + T @ T.mT
    return cov


def fit(make, dev):
    torch.manual_seed(0)
    net, xshape, nb = make()
    net = net.to(dev)
    kfac = KFAC(net)
    for _ in range(3):
        x = torch.rand(256, *xshape, device=dev)
        logits = net(x)
        y = torch.distributions.Categorical(logits=logits).sample()
        net.zero_grad()
        nn.functional.cross_entropy(logits, y).backward()
        kfac.update(256)
    kfac.invert(0.04, 200)
    layers = [m for m in list(net.modules())[1:] if m in kfac.state]
    return net, kfac, layers, torch.rand(nb, *xshape, device=dev), nb


def outer_terms(net, kfac, layers, x):
    _, io = layer_io_jacobians(net, layers, x)
    return [(a, D, *kfac.inv_state[l]) for l, (a, D) in zip(layers, io) if isinstance(l, nn.Linear)]


def run_factored_only(make, dev, args):
    net, kfac, layers, x, nb = fit(make, dev)
    terms = outer_terms(net, kfac, layers, x)
    res = {"nb": nb, "nc": terms[0][1].shape[1], "layers": [[t[2].shape[0], t[3].shape[0]] for t in terms]}
    res["cov_linear_outer_ms"] = event_ms(lambda: kron_covariance_outer(terms), args.warmup, args.reps)
    res["glm_factored_ms"] = event_ms(lambda: glm_predictive(kfac, x, chunk=nb, jacobians="factored"),
                                      args.warmup, args.reps)
    return res


def run(name, make, dev, args):
    net, kfac, layers, x, nb = fit(make, dev)
    _, Js = output_jacobians(net, layers, x)
    terms = [(J.contiguous(), *kfac.inv_state[l]) for l, J in zip(layers, Js)]
    nc = Js[0].shape[1]
    res = {"nb": nb, "nc": nc, "layers": [[t[1].shape[0], t[2].shape[0]] for t in terms]}
    res["apply_flops"] = sum(nb * nc * (a * a * g + a * g * g) for a, g in res["layers"])
    res["gram_bytes"] = sum(nb * nc * a * g * 4 for a, g in res["layers"])
    res["cov_ms"] = event_ms(lambda: kron_covariance(terms), args.warmup, args.reps)
    if args.only == "cov":
        return res
    res["torch_cov_ms"] = event_ms(lambda: torch_cov(terms), args.warmup, args.reps)
    got, want = kron_covariance(terms), torch_cov(terms)
    res["max_diff_vs_torch_over_max"] = float((got - want).abs().max() / want.abs().max())
    lin = [t for l, t in zip(layers, terms) if isinstance(l, nn.Linear)]
    outer = outer_terms(net, kfac, layers, x)
    res["cov_linear_dense_ms"], res["cov_linear_outer_ms"] = alternate_ms(
        [lambda: kron_covariance(lin), lambda: kron_covariance_outer(outer)], args.warmup, args.reps)
    res["glm_dense_ms"], res["glm_factored_ms"] = alternate_ms(
        [lambda: glm_predictive(kfac, x, chunk=nb),
         lambda: glm_predictive(kfac, x, chunk=nb, jacobians="factored")], args.warmup, args.reps)
    dense_cov = glm_predictive(kfac, x, chunk=nb)[1]
    fact_cov = glm_predictive(kfac, x, chunk=nb, jacobians="factored")[1]
    res["factored_max_diff_over_max"] = float((dense_cov - fact_cov).abs().max() / dense_cov.abs().max())
    res["glm_ms"] = event_ms(lambda: glm_predictive(kfac, x, chunk=nb), 2, max(3, args.reps // 4))

    def torch_glm():
        _, Jt = output_jacobians(net, layers, x)
        return torch_cov([(J, *kfac.inv_state[l]) for l, J in zip(layers, Jt)])

    res["torch_glm_ms"] = event_ms(torch_glm, 2, max(3, args.reps // 4))
    torch.set_num_threads(16)
    cpu_terms = [tuple(t.cpu() for t in term) for term in terms]
    torch_cov(cpu_terms)
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        torch_cov(cpu_terms)
        times.append((time.perf_counter() - t0) * 1e3)
    res["cpu_cov_ms"] = statistics.median(times)
    res["cpu_threads"] = torch.get_num_threads()
    return res


def damping_grid(nt):
    """nt dampings (add, multiply): add log-spaced over 1e-4 .. 1 at multiply 200."""
    return [(10.0 ** (-4.0 + 4.0 * i / max(1, nt - 1)), 200.0) for i in range(nt)]


def run_sweep(make, route, dev, args):
    net, kfac, layers, x, nb = fit(make, dev)
    res = {"nb": nb, "route": route, "layers": [[A.shape[0], G.shape[0]] for A, G in kfac.state.values()]}

    def eigh():
        kfac._eig_state = None
        kfac.eigh()

    res["eigh_ms"] = event_ms(eigh, 1, 3)
    eig = kfac.eigh()
    if route == "factored":
        _, io = layer_io_jacobians(net, layers, x)
        fixed = [(a, D) for a, D in io]
        plain, sweep = kron_covariance_outer, kron_covariance_outer_sweep
    else:
        fixed = [(J.contiguous(),) for J in output_jacobians(net, layers, x)[1]]
        plain, sweep = kron_covariance, kron_covariance_sweep
    sizes = sorted({1, 4, 16, args.sweep})
    for key in ("sweep_ms", "loop_ms", "sweep_cov_ms", "loop_cov_ms"):
        res[key] = {}
    for nt in sizes:
        grid = damping_grid(nt)

        def loop():
            out = []
            for add, multiply in grid:
                kfac.invert(add, multiply)
                out.append(glm_predictive(kfac, x, chunk=nb, jacobians=route)[1])
            return out

        sweep_terms = [(*f, eig[l][0][1], eig[l][1][1], damping_weights(eig[l][0][0], grid),
                        damping_weights(eig[l][1][0], grid)) for l, f in zip(layers, fixed)]
        kfac.invert(*grid[0])
        loop_terms = [(*f, *kfac.inv_state[l]) for l, f in zip(layers, fixed)]

        def loop_cov():
            for _ in grid:
                plain(loop_terms)

        reps = max(3, args.reps // (1 + nt // 4))
        res["sweep_ms"][nt], res["loop_ms"][nt], res["sweep_cov_ms"][nt], res["loop_cov_ms"][nt] = alternate_ms(
            [lambda: glm_predictive_sweep(kfac, x, grid, chunk=nb, jacobians=route), loop,
             lambda: sweep(sweep_terms), loop_cov], args.warmup if nt <= 4 else 2, reps)
        if nt == sizes[-1]:
            got = glm_predictive_sweep(kfac, x, grid, chunk=nb, jacobians=route)[1]
            want = torch.stack(loop())
            res["sweep_max_diff_over_max"] = float(((got - want).abs().amax(dim=(1, 2, 3)) /
                                                    want.abs().amax(dim=(1, 2, 3))).max())
    res["marginal_ms_per_damping"] = (res["sweep_ms"][16] - res["sweep_ms"][1]) / 15
    res["loop_ms_per_damping"] = res["loop_ms"][16] / 16
    res["marginal_cov_ms_per_damping"] = (res["sweep_cov_ms"][16] - res["sweep_cov_ms"][1]) / 15
    res["loop_cov_ms_per_damping"] = res["loop_cov_ms"][16] / 16
    return res


PEAK_FP32_MFMA_TFLOPS = 157.3


def torch_cov_joint(terms):
    cov = 0
    for J, LA, LG in terms:
        nA, nG = LA.shape[0], LG.shape[0]
        T = (LA.T @ J.view(-1, nA, nG) @ LG).flatten(1)
        cov = cov + T @ T.mT
    return cov


def torch_cov_outer_joint(terms):
    cov = 0
    for a, D, LA, LG in terms:
        nc = D.shape[1]
        abar = torch.cat([a, a.new_ones(a.shape[0], 1)], dim=1) if LA.shape[0] == a.shape[1] + 1 else a
        U, V = abar @ LA, D.flatten(0, 1) @ LG
        S = (U @ U.mT).repeat_interleave(nc, dim=0).repeat_interleave(nc, dim=1)
        cov = cov + S * (V @ V.mT)
    return cov


def run_joint(make, routes, dev, args):
    net, kfac, layers, x, nb = fit(make, dev)
    res = {"nb": nb, "layers": [[A.shape[0], G.shape[0]] for A, G in kfac.state.values()]}
    for route in routes:
        if route == "dense":
            _, Js = output_jacobians(net, layers, x)
            terms = [(J.contiguous(), *kfac.inv_state[l]) for l, J in zip(layers, Js)]
            joint, composed, per_sample = kron_covariance_joint, torch_cov_joint, kron_covariance
            R = nb * Js[0].shape[1]
            r = {"R": R, "gram_flops": sum(R * (R + 1) * t[1].shape[0] * t[2].shape[0] for t in terms),
                 "gram_bytes": sum(4 * R * t[1].shape[0] * t[2].shape[0] for t in terms)}
        else:
            terms = outer_terms(net, kfac, layers, x)
            joint, composed, per_sample = kron_covariance_outer_joint, torch_cov_outer_joint, kron_covariance_outer
            r = {"R": nb * terms[0][1].shape[1], "linear_layers": len(terms)}
        if args.only == "cov":
            r["joint_ms"] = event_ms(lambda: joint(terms), args.warmup, args.reps)
        else:
            r["joint_ms"], r["torch_ms"], r["per_sample_ms"] = alternate_ms(
                [lambda: joint(terms), lambda: composed(terms), lambda: per_sample(terms)], args.warmup, args.reps)
            got, want = joint(terms), composed(terms)
            r["max_diff_vs_torch_over_max"] = float((got.view_as(want) - want).abs().max() / want.abs().max())
            r["glm_joint_ms"] = event_ms(lambda: glm_predictive(kfac, x, chunk=min(nb, 64), jacobians=route,
                                                                joint=True), args.warmup, args.reps)
        if route == "dense":
            r["gram_tflops_of_call"] = r["gram_flops"] / (r["joint_ms"] * 1e-3) / 1e12
            r["gram_peak_fraction_of_call"] = r["gram_tflops_of_call"] / PEAK_FP32_MFMA_TFLOPS
            r["gram_gbytes_per_s_of_call"] = r["gram_bytes"] / (r["joint_ms"] * 1e-3) / 1e9
        res[route] = r
    return res


def lenet5():
    return nn.Sequential(nn.Conv2d(1, 6, 5, padding=2), nn.ReLU(), nn.MaxPool2d(2), nn.Conv2d(6, 16, 5), nn.ReLU(),
                         nn.MaxPool2d(2), nn.Flatten(), nn.Linear(400, 120), nn.ReLU(), nn.Linear(120, 84),
                         nn.ReLU(), nn.Linear(84, 10)), (1, 28, 28), 64


def run_conv_rows(make, dev, args):
    """The Conv2d rows of the factored route: the device call against torch's rows on the same
    captures, then glm_predictive end to end three ways, alternated call by call -- factored
    with the device rows, factored with torch's rows (the route as it was before the device
    rows: variance._conv_rows pointed at conv_jacobian_rows) and dense."""
    net, kfac, layers, x, nb = fit(make, dev)
    _, io = layer_io_jacobians(net, layers, x)
    convs = [(l, a, D) for l, (a, D) in zip(layers, io) if isinstance(l, nn.Conv2d)]
    nc = convs[0][2].shape[1]
    res = {"nb": nb, "nc": nc, "conv_layers": []}
    flops = 0
    for l, a, D in convs:
        nA = l.in_channels * l.kernel_size[0] * l.kernel_size[1] + (l.bias is not None)
        nG, L = D.shape[2], D.shape[3] * D.shape[4]
        flops += 2 * nA * nG * L * nb * nc
        dev_ms, torch_ms = alternate_ms([lambda: V.conv_jacobian_rows_device(l, a, D),
                                         lambda: V.conv_jacobian_rows(l, a, D)], args.warmup, args.reps)
        got, want = V.conv_jacobian_rows_device(l, a, D), V.conv_jacobian_rows(l, a, D)
        res["conv_layers"].append({"nA": nA, "nG": nG, "L": L, "tasks": nb * -(-nA // 64) * -(-nc * nG // 64),
                                   "rows_device_ms": dev_ms, "rows_torch_ms": torch_ms,
                                   "max_diff_over_max": float((got - want).abs().max() / want.abs().max())})
    res["rows_flops"] = flops
    res["rows_device_ms"], res["rows_torch_ms"] = alternate_ms(
        [lambda: [V.conv_jacobian_rows_device(l, a, D) for l, a, D in convs],
         lambda: [V.conv_jacobian_rows(l, a, D) for l, a, D in convs]], args.warmup, args.reps)
    res["rows_device_tflops"] = flops / (res["rows_device_ms"] * 1e-3) / 1e12
    if args.only == "cov":
        return res
    device_rows = V._conv_rows

    def factored(rows):
        def call():
            V._conv_rows = rows
            try:
                return glm_predictive(kfac, x, chunk=nb, jacobians="factored")
            finally:
                V._conv_rows = device_rows
        return call

    res["glm_factored_device_rows_ms"], res["glm_factored_torch_rows_ms"], res["glm_dense_ms"] = alternate_ms(
        [factored(device_rows), factored(V.conv_jacobian_rows), lambda: glm_predictive(kfac, x, chunk=nb)],
        args.warmup, args.reps)
    new, old = factored(device_rows)()[1], factored(V.conv_jacobian_rows)()[1]
    dense = glm_predictive(kfac, x, chunk=nb)[1]
    res["device_vs_torch_rows_max_diff_over_max"] = float((new - old).abs().max() / old.abs().max())
    res["factored_vs_dense_max_diff_over_max"] = float((new - dense).abs().max() / dense.abs().max())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="mlp,basenet15k,c5",
                    help="--sweep / --joint: which of mlp, basenet15k, c5 to run (one JSON line each, then the whole)")
    ap.add_argument("--sweep", type=int, default=0, metavar="NT",
                    help="time the damping grid (glm_predictive_sweep) at 1, 4, 16 and NT dampings instead")
    ap.add_argument("--joint", action="store_true",
                    help="time the joint covariance across the samples (glm_predictive(joint=True)) instead")
    ap.add_argument("--conv-rows", action="store_true",
                    help="time the Conv2d rows of the factored route (conv_jacobian_rows_device against torch's "
                         "rows, glm_predictive end to end with either and dense) on basenet15k and lenet5 instead")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["all", "cov"], default="all",
                    help="cov: kron_covariance (--joint: the joint call) alone (A/B builds, profiler runs)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"workload": "GLM predictive covariance", "lib": N.LIB_PATH}
    if args.conv_rows:
        out["workload"] = "Conv2d Jacobian rows of the factored GLM predictive"
        for name, make in (("basenet15k", basenet15k), ("lenet5", lenet5)):
            out[name] = run_conv_rows(make, dev, args)
            print(json.dumps({name: out[name]}), flush=True)
        print(json.dumps(out))
        return
    if args.sweep:
        out["workload"] = "GLM predictive over a damping grid"
        for name, make, route in (("mlp", mlp, "factored"), ("basenet15k", basenet15k, "dense"),
                                  ("c5", c5, "factored")):
            if name in args.workloads.split(","):
                out[name] = run_sweep(make, route, dev, args)
                print(json.dumps({name: out[name]}), flush=True)
        print(json.dumps(out))
        return
    if args.joint:
        out["workload"] = "joint GLM predictive covariance"
        for name, make, routes in (("mlp", mlp, ("dense", "factored")),
                                   ("basenet15k", basenet15k, ("dense", "factored")), ("c5", c5, ("factored",))):
            if name in args.workloads.split(","):
                out[name] = run_joint(make, routes, dev, args)
                print(json.dumps({name: out[name]}), flush=True)
        print(json.dumps(out))
        return
    for name, make in (("mlp", mlp), ("basenet15k", basenet15k)):
        out[name] = run(name, make, dev, args)
    if args.only == "all":
        out["c5"] = run_factored_only(c5, dev, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
