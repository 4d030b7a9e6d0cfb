"""Inputs and fp64 references shared by the damping-sweep tests (test_gpu_glm_sweep.py,
test_glm_sweep_host.py).  Every reference is numpy fp64 computed from the same fp32 inputs
the device gets, once per shape (lru_cache, arrays read-only)."""
import copy
import functools

import numpy as np
import torch
import torch.nn as nn

NT_MAX = 64
ONES_ROW = 1  # the grid point whose weights are all 1 (needs nt >= 2)


def _orthogonal(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return q.astype(np.float32)


def _weights(rng, n):
    """(NT_MAX, n) positive fp32 weights spread over 1e6, row ONES_ROW all ones."""
    w = (10.0 ** rng.uniform(-3.0, 3.0, size=(NT_MAX, n))).astype(np.float32)
    w[:, 0] = np.float32(1e-3)
    w[:, -1] = np.float32(1e3) if n > 1 else w[:, -1]
    w[ONES_ROW] = 1.0
    return w


def _freeze(*arrays):
    for t in arrays:
        t.setflags(write=False)
    return arrays


def outer_ref(a, ones, D, VA, VG, wA, wG):
    a, D, VA, VG, wA, wG = (t.astype(np.float64) for t in (a, D, VA, VG, wA, wG))
    abar = np.concatenate([a, np.ones((a.shape[0], 1))], axis=1) if ones else a
    s = ((abar @ VA) ** 2) @ wA.T                      # (nb, nt)
    Q = D @ VG                                         # (nb, nc, nG)
    gram = np.einsum("bcg,tg,bdg->tbcd", Q, wG, Q)
    return s.T[:, :, None, None] * gram


def dense_ref(J, nA, nG, VA, VG, wA, wG):
    J, VA, VG, wA, wG = (t.astype(np.float64) for t in (J, VA, VG, wA, wG))
    nb, nc = J.shape[:2]
    Y = np.einsum("ai,bcag,gh->bcih", VA, J.reshape(nb, nc, nA, nG), VG)
    return np.einsum("ti,th,bcih,bdih->tbcd", wA, wG, Y, Y)


@functools.lru_cache(maxsize=None)
def outer_case(cols, ones, nG, nb, nc, seed=0):
    """(a, D, VA, VG, wA, wG) fp32 and the fp64 reference (NT_MAX, nb, nc, nc)."""
    rng = np.random.default_rng(seed + 1000 * cols + nG)
    nA = cols + ones
    a = rng.standard_normal((nb, cols)).astype(np.float32)
    D = rng.standard_normal((nb, nc, nG)).astype(np.float32)
    VA, VG = _orthogonal(rng, nA), _orthogonal(rng, nG)
    wA, wG = _weights(rng, nA), _weights(rng, nG)
    return _freeze(a, D, VA, VG, wA, wG, outer_ref(a, ones, D, VA, VG, wA, wG))


@functools.lru_cache(maxsize=None)
def dense_case(nA, nG, nb, nc, seed=0):
    """(J, VA, VG, wA, wG) fp32 and the fp64 reference (NT_MAX, nb, nc, nc)."""
    rng = np.random.default_rng(seed + 1000 * nA + nG)
    J = rng.standard_normal((nb, nc, nA * nG)).astype(np.float32)
    VA, VG = _orthogonal(rng, nA), _orthogonal(rng, nG)
    wA, wG = _weights(rng, nA), _weights(rng, nG)
    return _freeze(J, VA, VG, wA, wG, dense_ref(J, nA, nG, VA, VG, wA, wG))


def factor_shaped(n, ones, seed):
    """A symmetric PSD fp32 matrix shaped like a KFAC factor: a second moment of fewer
    samples than columns (rank-deficient), with the ones column of a bias when asked."""
    rng = np.random.default_rng(seed)
    X = np.maximum(rng.standard_normal((max(2, n // 2), n)), 0.0)
    if ones:
        X[:, -1] = 1.0
    F = (X.T @ X / X.shape[0]).astype(np.float32)
    return ((F + F.T) / 2).astype(np.float32)


# ------------------------------------------------------------------ end to end
def categorical_loss(out):
    y = torch.distributions.Categorical(logits=out.detach()).sample()
    return torch.nn.functional.cross_entropy(out, y)


def regression_loss(out):
    return ((out - torch.randn_like(out)) ** 2).mean()


def small_nets():
    """name -> (constructor, input shape, loss): the nets of the existing GLM tests."""
    from models_for_tests import BaseNet750
    return {"no_bias": (lambda: nn.Sequential(nn.Linear(12, 7, bias=False), nn.Tanh(), nn.Linear(7, 3)),
                        (12,), categorical_loss),
            "regression": (lambda: nn.Sequential(nn.Linear(4, 8), nn.Tanh(), nn.Linear(8, 1)),
                           (4,), regression_loss),
            "relu_inplace": (lambda: nn.Sequential(nn.Linear(9, 6), nn.ReLU(inplace=True), nn.Linear(6, 4)),
                             (9,), categorical_loss),
            "basenet750": (BaseNet750, (1, 28, 28), categorical_loss)}


def fit(dev, net, make_x, loss_of, passes=3):
    """(net on dev, its fp64 CPU copy, KFAC after `passes` updates of 64 samples)."""
    from bnn_kfac_amd.curvatures import KFAC
    net64 = copy.deepcopy(net).double()  # (before KFAC hooks the modules)
    net = net.to(dev)
    kfac = KFAC(net)
    for _ in range(passes):
        out = net(make_x(64))
        net.zero_grad()
        loss_of(out).backward()
        kfac.update(64)
    return net, net64, kfac


def grid_for(count):
    """The issue's grid: three scalar pairs and one per-layer pair of lists."""
    return [(0.04, 200.0), (1.0, 200.0), (1e-4, 1.0),
            ([0.04 * (i + 1) for i in range(count)], [200.0 / (i + 1) for i in range(count)])]


def point_of(grid_point, index):
    add, multiply = grid_point
    return (add[index], multiply[index]) if isinstance(add, (list, tuple)) else (add, multiply)


def fp64_rows(net64, layers64, x):
    """(logits (n, nc), [M_l (n, nc, nA, nG)]): Jacobian rows in the posterior's order by
    autograd on the fp64 CPU copy (M[a][g] = dW[g][a], bias row last)."""
    logits, rows = [], [[] for _ in layers64]
    for b in range(x.shape[0]):
        out = net64(x[b:b + 1].double())[0]
        per = [[] for _ in layers64]
        for c in range(out.shape[0]):
            net64.zero_grad()
            out[c].backward(retain_graph=True)
            for li, layer in enumerate(layers64):
                dW = layer.weight.grad.numpy()
                M = dW.reshape(dW.shape[0], -1).T
                if layer.bias is not None:
                    M = np.concatenate([M, layer.bias.grad.numpy()[None, :]], axis=0)
                per[li].append(M.copy())
        for li in range(len(layers64)):
            rows[li].append(np.stack(per[li]))
        logits.append(out.detach().numpy())
    return np.stack(logits), [np.stack(r) for r in rows]


def fp64_cov(rows, factors64, points):
    """cov (n, nc, nc) = sum_l <M, inverse(sqrt(s) A + sqrt(n) I) M inverse(sqrt(s) G + sqrt(n) I)>
    with layer l's (add n, multiply s) = points[l]; factors64 = [(A, G)] fp64."""
    cov = 0.0
    for M, (A, G), (n, s) in zip(rows, factors64, points):
        SA = np.linalg.inv(np.sqrt(s) * A + np.sqrt(n) * np.eye(A.shape[0]))
        SG = np.linalg.inv(np.sqrt(s) * G + np.sqrt(n) * np.eye(G.shape[0]))
        cov = cov + np.einsum("bcag,ai,gh,bdih->bcd", M, SA, SG, M)
    return cov


def fp32_eigen_cov(rows, factors64, points):
    """The eigen route as the device evaluates it, emulated on the host: eigenpairs of the
    fp32 factors, V and the weights rounded to fp32, fp32 products and sums."""
    cov = 0.0
    for M, (A, G), (n, s) in zip(rows, factors64, points):
        parts = []
        for F_ in (A, G):
            lam, V = np.linalg.eigh((F_ + F_.T) / 2)
            parts.append((V.astype(np.float32), (1.0 / (np.sqrt(s) * lam + np.sqrt(n))).astype(np.float32)))
        (VA, wA), (VG, wG) = parts
        Y = np.einsum("ai,bcag,gh->bcih", VA, M.astype(np.float32), VG).astype(np.float32)
        cov = cov + np.einsum("i,h,bcih,bdih->bcd", wA, wG, Y, Y).astype(np.float32)
    return cov
