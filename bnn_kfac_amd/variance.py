"""Sampling-free predictive variance with Kronecker-factored posteriors.

Replaces the per-layer `J_i @ torch.kron(Q_i, H_i) @ J_i.t()` loops of
sampling_free/classification/classification_ll_block.py:114-170 and
sampling_free/regression/regression_ll_block.py:120-140 with one grouped device
contraction (libkfac_hip `kfac_kron_quadform`) that never forms the Kronecker
product.  The Jacobians J themselves stay host-side PyTorch autograd, exactly as
the reference builds them (sampling_free/utils.py:221-226).

The GLM predictive (glm_predictive / probit_predictive, further down) goes beyond the
reference: logits and their full covariance under the KFAC posterior in closed form
(`kfac_kron_cov`; above 32 outputs `kfac_kron_cov_tiled`), where the reference samples weights
and re-runs the network.
"""
from __future__ import annotations

import contextlib
import math
from collections import OrderedDict
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _native as N


def gradient(y: Tensor, x: Tensor, grad_outputs: Tensor = None) -> Tensor:
    """dy/dx @ grad_outputs (sampling_free/utils.py:221-226)."""
    if grad_outputs is None:
        grad_outputs = torch.ones_like(y)
    return torch.autograd.grad(y, [x], grad_outputs=grad_outputs, create_graph=True,
                               retain_graph=True, allow_unused=True)[0]


def layer_jacobian(output: Tensor, layer: torch.nn.Module, grad_outputs: Tensor) -> Tensor:
    """J_i = cat([flatten(dW), flatten(db)]) (classification_ll_block.py:128-130)."""
    g = [torch.flatten(gradient(output, p, grad_outputs)) for p in layer.parameters()]
    return torch.cat(g, dim=0)


def kron_quadform(terms: Sequence[Tuple[Tensor, Tensor, Tensor]], lower: bool = True,
                  abs_sum: bool = True, per_term: bool = False):
    """sum_l |J_l kron(K1_l, K2_l) J_l^T| for rows of J_l (shape (nb, nA*nG) or (nA*nG,)).

    terms: [(J_l, K1_l, K2_l)], K1 (nA x nA), K2 (nG x nG), J in the reference's flat
    order a*nG + g.  `lower` marks K1/K2 as lower-triangular (Cholesky factors from
    KFAC.invert) so their zero blocks are skipped.  Returns out (nb,) fp32 and, if
    per_term, the raw per-layer values (L, nb).
    """
    if not terms:
        raise ValueError("no terms")
    Js = []
    nb = None
    for J, K1, K2 in terms:
        J2 = J.detach()
        J2 = J2.reshape(1, -1) if J2.dim() == 1 else J2
        if J2.stride(-1) != 1:
            J2 = J2.contiguous()
        if nb is None:
            nb = J2.shape[0]
        elif J2.shape[0] != nb:
            raise ValueError("all terms need the same number of rows")
        Js.append(J2)
    device = Js[0].device
    out = torch.empty(nb, dtype=torch.float32, device=device)
    v = torch.empty(len(terms), nb, dtype=torch.float32, device=device) if per_term else None
    keep = []
    groups = []
    for li, ((_, K1, K2), J2) in enumerate(zip(terms, Js)):
        nA, nG = K1.shape[0], K2.shape[0]
        if J2.shape[1] != nA * nG:
            raise ValueError(f"J has {J2.shape[1]} columns, kron(K1, K2) needs {nA * nG}")
        for t, what in ((J2, "J"), (K1, "K1"), (K2, "K2")):
            N.require_device(t, what)
        K1c = K1.detach() if K1.stride(-1) == 1 else K1.detach().contiguous()
        K2c = K2.detach() if K2.stride(-1) == 1 else K2.detach().contiguous()
        keep.extend([K1c, K2c])
        q = N.QuadJob()
        q.J, q.ldJ, q.nA, q.nG = J2.data_ptr(), J2.stride(0) if nb > 1 else nA * nG, nA, nG
        q.K1, q.ld1, q.K2, q.ld2 = K1c.data_ptr(), K1c.stride(0), K2c.data_ptr(), K2c.stride(0)
        q.lower1 = q.lower2 = int(lower)
        q.v = v[li].data_ptr() if per_term else 0
        groups.append(q)
    # the C-ABI groups up to 8 terms per launch; fold larger models in chunks
    if len(groups) <= 8:
        N.kron_quadform(groups, nb, abs_sum, out)
    else:
        acc = torch.zeros(nb, dtype=torch.float32, device=device)
        for g0 in range(0, len(groups), 8):
            part = torch.empty(nb, dtype=torch.float32, device=device)
            N.kron_quadform(groups[g0:g0 + 8], nb, abs_sum, part)
            acc += part
        out = acc
    return (out, v) if per_term else out


@contextlib.contextmanager
def hooks_suspended(model: torch.nn.Module):
    """KFAC's module hooks (record capture) must not fire inside the functorch
    transforms: suspend every module hook of `model` inside the block, then restore
    the exact hook dictionaries."""
    kinds = ("_forward_hooks", "_forward_pre_hooks", "_backward_hooks", "_backward_pre_hooks")
    saved = [(m, [getattr(m, k) for k in kinds]) for m in model.modules()]
    for m, _ in saved:
        for k in kinds:
            setattr(m, k, OrderedDict())
    try:
        yield
    finally:
        for m, dicts in saved:
            for k, d in zip(kinds, dicts):
                setattr(m, k, d)


def layer_jacobians(output: Tensor, layers: Sequence[torch.nn.Module], grad_outputs: Tensor) -> List[Tensor]:
    """[J_i] for several layers from ONE backward pass: the same vectors as the
    reference's per-parameter `gradient` calls (classification_ll_block.py:128-130,
    sampling_free/utils.py:221-226), which each run a full backward."""
    params = [p for layer in layers for p in layer.parameters()]
    grads = torch.autograd.grad(output, params, grad_outputs=grad_outputs, retain_graph=True,
                                allow_unused=True)
    out, k = [], 0
    for layer in layers:
        n = len(list(layer.parameters()))
        out.append(torch.cat([torch.flatten(g) for g in grads[k:k + n]], dim=0))
        k += n
    return out


def kfac_predictive_std(kfac, output: Tensor, grad_outputs: Tensor, layers: Iterable = None,
                        per_layer: bool = False):
    """The reference's `pred_std` for one test batch (classification_ll_block.py:118-132):
    sum over KFAC layers of |J_i kron(L_A, L_G) J_i^T|, J_i the gradient of
    `output` weighted by `grad_outputs` w.r.t. the layer's [W, b]."""
    if layers is None:
        layers = [m for m in list(kfac.model.modules())[1:] if m in kfac.state]
    layers = list(layers)
    terms = []
    for layer, J in zip(layers, layer_jacobians(output, layers, grad_outputs)):
        LA, LG = kfac.inv_state[layer]
        terms.append((J, LA, LG))
    res = kron_quadform(terms, lower=True, abs_sum=True, per_term=per_layer)
    if per_layer:
        return float(res[0][0]), res[1][:, 0]
    return float(res[0])


def per_sample_predictive_std(kfac, x: Tensor, layers: Iterable = None, chunk: int = 256) -> Tensor:
    """Predictive std of every sample of `x` as the reference computes it for a test
    batch of ONE image (classification_ll_block.py:114-135 / the noise loop 147-165):
    p = softmax(net(x_b)), grad_outputs = one-hot(argmax p), J_l = d(go . p)/d[W_l, b_l],
    std_b = sum_l |J_l kron(L_A, L_G) J_l^T|.

    Per-sample Jacobians come from ONE vmapped gradient per chunk (torch.func), and
    the whole chunk is contracted by a single kfac_kron_quadform launch (nb rows per
    layer) instead of a Python loop of single-image backward passes.  Returns (N,) fp32.
    """
    from torch.func import functional_call, grad, vmap
    model = kfac.model
    if layers is None:
        layers = [m for m in list(model.modules())[1:] if m in kfac.state]
    layers = list(layers)
    names = {id(p): n for n, p in model.named_parameters()}
    pnames = [[names[id(p)] for p in layer.parameters()] for layer in layers]
    with hooks_suspended(model):
        return _per_sample_std(kfac, model, layers, pnames, x, chunk, functional_call, grad, vmap)


def _per_sample_std(kfac, model, layers, pnames, x, chunk, functional_call, grad, vmap):
    flat = [n for group in pnames for n in group]
    params = {n: p.detach() for n, p in model.named_parameters()}
    buffers = {n: b for n, b in model.named_buffers()}

    def score(theta, xb):
        full = dict(params)
        full.update(theta)
        p = torch.softmax(functional_call(model, (full, buffers), (xb.unsqueeze(0),)), dim=1)[0]
        go = (p == p.max()).to(p.dtype)  # one-hot argmax (a comparison: no gradient through it)
        return (go.detach() * p).sum()

    jac = vmap(grad(score), in_dims=(None, 0))
    out = []
    for c0 in range(0, x.shape[0], chunk):
        g = jac({n: params[n] for n in flat}, x[c0:c0 + chunk])
        terms = []
        for layer, group in zip(layers, pnames):
            J = torch.cat([g[n].reshape(g[n].shape[0], -1) for n in group], dim=1)
            LA, LG = kfac.inv_state[layer]
            terms.append((J, LA, LG))
        out.append(kron_quadform(terms, lower=True, abs_sum=True))
    return torch.cat(out)


# ------------------------------------------------------------ GLM predictive
# The closed-form counterpart of the sampling loop (sampling/classification_sampling.py:
# 71-79: sample_and_replace + a forward pass per draw): logits f(x) and their full
# covariance J Sigma J^T under the Gaussian KFAC.sample draws from, by kfac_kron_cov.
MAX_COV_CLASSES = 32


def posterior_jacobian(dW: Tensor, db: Tensor = None, batch_dims: int = None) -> Tensor:
    """Jacobian rows in the posterior's order: KFAC.sample draws S (nA x nG) and adds
    S^T into [W | b], so row M (nA x nG, flat index a*nG + g) has M[a][g] = dW[g][a]
    for a < wcols and M[nA-1][g] = db[g].

    dW: (..., nG, *rest) (a Conv2d weight is flattened per output channel, F.unfold's
    column order), db: (..., nG) or None.  `batch_dims` leading dimensions are kept
    (default: db.dim() - 1, or 0 without db).  Returns (..., nA*nG).  Pure torch.
    """
    if batch_dims is None:
        batch_dims = db.dim() - 1 if db is not None else 0
    if dW.dim() < batch_dims + 1:
        raise ValueError(f"dW {tuple(dW.shape)} has no nG dimension after {batch_dims} batch dimensions")
    lead = tuple(dW.shape[:batch_dims])
    nG = dW.shape[batch_dims]
    M = dW.reshape(*lead, nG, -1).transpose(-1, -2)  # (..., wcols, nG)
    if db is not None:
        if tuple(db.shape) != lead + (nG,):
            raise ValueError(f"db {tuple(db.shape)} does not match dW {tuple(dW.shape)}")
        M = torch.cat([M, db.unsqueeze(-2)], dim=-2)
    return M.reshape(*lead, -1)


def _cov_rows(J: Tensor, K: int):
    """(J as (nb, nc, K) with rows r = b*nc + c a constant stride apart, that stride)."""
    J = J.detach()
    if J.dim() == 2:
        J = J.unsqueeze(0)
    if J.dim() != 3 or J.shape[2] != K:
        raise ValueError(f"J {tuple(J.shape)}: expected (nb, nc, {K}) or (nc, {K})")
    nb, nc = J.shape[0], J.shape[1]
    ld = J.stride(1) if nc > 1 else (J.stride(0) if nb > 1 else K)
    if J.stride(2) != 1 or ld < K or (nb > 1 and J.stride(0) != nc * ld):
        J, ld = J.contiguous(), K
    return J, ld


def _rows_head(J: Tensor, nA: int, nG: int):
    """The head of a term given by its Jacobian rows J, (nb, nc, nA*nG) or (nc, nA*nG).  The shape
    phase happens here (_cov_rows); returns (nb, nc, None, fields), `fields(keep)` the device
    phase: the job tuple's first four fields (J, ldJ, nA, nG), J joining `keep`."""
    J3, ld = _cov_rows(J, nA * nG)

    def fields(keep):
        N.require_device(J3, "J")
        keep.append(J3)
        return J3.data_ptr(), ld, nA, nG

    return J3.shape[0], J3.shape[1], None, fields


def _outer_head(a: Tensor, D: Tensor, nA: int, nG: int, factor: str, F: Tensor):
    """The head of a Linear layer's term given by (a, D) in place of its rows: a (nb, cols) or
    (cols,), D (nb, nc, nG) or (nc, nG), nA = cols + 1 (the ones column is implicit) or cols;
    `factor`, `F`: name and tensor of the A-side factor, for the message.  The shape phase
    happens here; returns (nb, nc, a's rows, fields), `fields(keep)` the device phase: the job
    tuple's first eight fields (a, lda, cols, has_ones, D, ldD, nG, 0), a (copied unless its rows
    have unit stride and do not overlap) and D joining `keep`."""
    D3, ldD = _cov_rows(D, nG)
    a2 = a.detach()
    a2 = a2.reshape(1, -1) if a2.dim() == 1 else a2
    if a2.dim() != 2:
        raise ValueError(f"a {tuple(a2.shape)}: expected (nb, cols), a Linear layer's 2-D input")
    cols = a2.shape[1]
    if nA not in (cols, cols + 1) or cols == 0:
        raise ValueError(f"a has {cols} columns, {factor} {tuple(F.shape)} needs {nA} or {nA - 1}")
    nb = D3.shape[0]

    def fields(keep):
        ac = a2.contiguous() if a2.stride(1) != 1 or (nb > 1 and a2.stride(0) < cols) else a2
        lda = ac.stride(0) if nb > 1 else cols
        for t, what in ((ac, "a"), (D3, "D")):
            N.require_device(t, what)
        keep.extend([ac, D3])
        return ac.data_ptr(), lda, cols, int(nA == cols + 1), D3.data_ptr(), ldD, nG, 0

    return nb, D3.shape[1], a2.shape[0], fields


def _parse_terms(terms, shapes, who: str, max_classes, weights: str = None):
    """The term loop every builder shares, shapes only (nothing touches the device):
    `shapes(term)` -> (head (_rows_head / _outer_head), what the device phase needs of the tail,
    the grid sizes of the tail's weights).  Establishes the common (nb, nc) and, for the weighted
    calls, nt (`weights`: what nt counts, for the message); `max_classes` None: no cap on nc.
    Returns ([(the head's device phase, tail)], nb, nc, nt)."""
    if not terms:
        raise ValueError("no terms")
    parsed = []
    nb = nc = nt = None
    for term in terms:
        (tnb, tnc, a_rows, fields), tail, counts = shapes(term)
        if nb is None:
            nb, nc, nt = tnb, tnc, counts[0] if counts else None
        elif (tnb, tnc) != (nb, nc):
            raise ValueError("all terms need the same (nb, nc)")
        if a_rows is not None and a_rows != nb:
            raise ValueError(f"a has {a_rows} rows, D has {nb} samples")
        if counts and (nt == 0 or counts.count(nt) != len(counts)):
            raise ValueError(f"all weights need the same number nt >= 1 of {weights}")
        if max_classes is not None and nc > max_classes:
            raise ValueError(f"{who} handles at most {max_classes} outputs, got {nc}")
        parsed.append((fields, tail))
    return parsed, nb, nc, nt


def _kron_jobs(terms, outer: bool, lower: bool, who: str, max_classes):
    """_cov_jobs (outer False) / _cov_outer_jobs (outer True)."""
    def shapes(term):
        if outer:
            a, D, K1, K2 = term
        else:
            J, K1, K2 = term
        if K1.dim() != 2 or K2.dim() != 2 or K1.shape[0] != K1.shape[1] or K2.shape[0] != K2.shape[1]:
            raise ValueError(f"K1 {tuple(K1.shape)} / K2 {tuple(K2.shape)}: expected square matrices")
        nA, nG = K1.shape[0], K2.shape[0]
        return (_outer_head(a, D, nA, nG, "K1", K1) if outer else _rows_head(J, nA, nG)), (K1, K2), ()

    parsed, nb, nc, _ = _parse_terms(terms, shapes, who, max_classes)
    keep, jobs = [], []
    for head, (K1, K2) in parsed:
        fields = head(keep)
        for t, what in ((K1, "K1"), (K2, "K2")):
            N.require_device(t, what)
        K1c = K1.detach() if K1.stride(-1) == 1 else K1.detach().contiguous()
        K2c = K2.detach() if K2.stride(-1) == 1 else K2.detach().contiguous()
        keep.extend([K1c, K2c])
        jobs.append((*fields, K1c.data_ptr(), K1c.stride(0), K2c.data_ptr(), K2c.stride(0), int(lower), int(lower)))
    return keep, jobs, nb, nc


def _cov_jobs(terms, lower: bool, who: str, max_classes: int = None):
    """(tensors to keep alive, kfac_cov_job tuples, nb, nc) of [(J_l, K1_l, K2_l)]."""
    return _kron_jobs(terms, False, lower, who, max_classes)


def _cov_job_at(j, b0: int, nc: int):
    """The kfac_cov_job tuple j with its rows starting at sample b0."""
    return (j[0] + 4 * b0 * nc * j[1], *j[1:])


def _run_per_sample(jobs, struct, job_at, workspace_bytes, call, nb, nc, device, max_workspace_bytes):
    """What the per-sample calls share: the (nb, nc, nc) result, jobs folded in groups of 8
    with `accumulate`, the samples cut into chunks that need at most `max_workspace_bytes` of
    scratch each (`job_at(j, b0, nc)`: job tuple j moved to sample b0)."""
    out = torch.empty(nb, nc, nc, dtype=torch.float32, device=device)
    if nb == 0:
        return out
    groups = [jobs[i:i + 8] for i in range(0, len(jobs), 8)]

    def need(n):
        return max(workspace_bytes([struct(*j) for j in g], n, nc) for g in groups)

    step = nb
    while step > 1 and need(step) > max_workspace_bytes:
        step = max(1, min(step - 1, step * max_workspace_bytes // need(step)))
    if need(step) > max_workspace_bytes:
        raise ValueError(f"one sample needs {need(1)} workspace bytes, max_workspace_bytes is "
                         f"{max_workspace_bytes}")
    for b0 in range(0, nb, step):
        n = min(step, nb - b0)
        for gi, g in enumerate(groups):
            call([struct(*job_at(j, b0, nc)) for j in g], n, nc, out[b0:b0 + n], accumulate=gi > 0)
    return out


def kron_covariance(terms: Sequence[Tuple[Tensor, Tensor, Tensor]], lower: bool = True,
                    max_workspace_bytes: int = 1 << 30) -> Tensor:
    """cov[b, c, c'] = sum_l J_l[b, c] (K1_l K1_l^T kron K2_l K2_l^T) J_l[b, c']^T.

    terms: [(J_l, K1_l, K2_l)], J (nb, nc, nA*nG) or (nc, nA*nG) in the POSTERIOR's order
    (posterior_jacobian), K1 (nA x nA), K2 (nG x nG); `lower` marks them lower-triangular
    (KFAC.invert's Cholesky factors).  Returns (nb, nc, nc) fp32, every block bitwise
    symmetric.  More than 8 terms fold in groups of 8; the samples are cut into chunks
    that need at most `max_workspace_bytes` of scratch each (a sample's block depends
    on that sample only, so chunking does not change a bit).  Shapes are checked
    (ValueError) before anything touches the device.
    """
    keep, jobs, nb, nc = _cov_jobs(terms, lower, "kron_covariance", MAX_COV_CLASSES)
    return _run_per_sample(jobs, N.CovJob, _cov_job_at, N.kron_cov_workspace_bytes, N.kron_cov, nb, nc,
                           keep[0].device, max_workspace_bytes)


def kron_covariance_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor]], lower: bool = True,
                          max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance for any number of outputs (a CIFAR-100 or ImageNet head): the same
    terms, the same (nb, nc, nc) fp32 result, nc not capped (kfac_kron_cov_tiled: a sample's
    block in 64x64 class tiles).

    Every block is bitwise symmetric, two calls give identical bits, terms fold in groups of
    8 and the samples are chunked under `max_workspace_bytes` without changing a bit, as in
    kron_covariance.  Block b has exactly the bits of kron_covariance_joint's block
    cov[b, :, b, :] on the same terms (marginal_blocks); against kron_covariance (nc <= 32,
    another summation order) it agrees to fp32 rounding.
    """
    keep, jobs, nb, nc = _cov_jobs(terms, lower, "kron_covariance_tiled")
    return _run_per_sample(jobs, N.CovJob, _cov_job_at, N.kron_cov_tiled_workspace_bytes,
                           N.kron_cov_tiled, nb, nc, keep[0].device, max_workspace_bytes)


def output_jacobians(model: torch.nn.Module, layers: Sequence[torch.nn.Module], x: Tensor):
    """(logits (n, nc), [J_l (n, nc, nA_l*nG_l)]): every sample's Jacobian of the model's
    outputs w.r.t. each layer's [W | b], in the posterior's order (posterior_jacobian),
    from one vmapped reverse-mode Jacobian (torch.func).  Module hooks are suspended."""
    from torch.func import functional_call, jacrev, vmap
    names = {id(p): n for n, p in model.named_parameters()}
    pnames = []
    for layer in layers:
        bias = getattr(layer, "bias", None)
        pnames.append((names[id(layer.weight)], names[id(bias)] if bias is not None else None))
    params = {n: p.detach() for n, p in model.named_parameters()}
    buffers = {n: b for n, b in model.named_buffers()}
    theta = {n: params[n] for group in pnames for n in group if n is not None}

    def outputs(th, xb):
        full = dict(params)
        full.update(th)
        y = functional_call(model, (full, buffers), (xb.unsqueeze(0),))[0].reshape(-1)
        return y, y

    with hooks_suspended(model):
        jac, logits = vmap(jacrev(outputs, has_aux=True), in_dims=(None, 0))(theta, x)
    Js = [posterior_jacobian(jac[w], jac[b] if b is not None else None, batch_dims=2)
          for w, b in pnames]
    return logits.detach(), Js


def layer_io_jacobians(model: torch.nn.Module, layers: Sequence[torch.nn.Module], x: Tensor):
    """(logits (n, nc), [(a_l, D_l)]): every layer's input a_l (n, ...) and the Jacobian of
    the model's outputs at the layer's output z_l, D_l (n, nc, *z_l.shape[1:]) contiguous
    with D_l[b, c] = d f_c(x_b) / d z_l[b], from ONE forward and one batched backward of
    the nc one-hot output vectors to all captured outputs.  For a Linear layer the
    Jacobian row w.r.t. [W | b] is outer([a_b | 1], D[b, c]): no row is materialised.

    Assumes independent samples (no train-mode BatchNorm: d f(x_b) / d z[b'] = 0 for
    b' != b) and that each layer is called once per forward.  Module hooks are suspended
    and restored.  Pure torch: works on CPU tensors."""
    layers = list(layers)
    captured = {}

    def capture(module, inputs, output):
        if module in captured:
            raise RuntimeError(f"{module.__class__.__name__} was called twice in one forward")
        captured[module] = (inputs[0].detach(), output)
        # the module's successor may work in place (nn.ReLU(inplace=True)): hand it a copy,
        # so the captured tensor stays the layer's own output z
        return output.clone()

    with hooks_suspended(model), torch.enable_grad():
        handles = [layer.register_forward_hook(capture) for layer in layers]
        try:
            xin = x.detach()
            if xin.is_floating_point():
                xin = xin.requires_grad_(True)  # (a frozen first layer still gets a graph)
            y = model(xin)
        finally:
            for h in handles:
                h.remove()
        missing = [l.__class__.__name__ for l in layers if l not in captured]
        if missing:
            raise RuntimeError(f"layers not reached by the forward pass: {missing}")
        n = y.shape[0]
        y = y.reshape(n, -1)
        nc = y.shape[1]
        zs = [captured[layer][1] for layer in layers]
        # grad_outputs[c] selects output c of every sample: samples are independent, so
        # d sum_b f_c(x_b) / d z[b] = d f_c(x_b) / d z[b]
        go = torch.zeros(nc, n, nc, dtype=y.dtype, device=y.device)
        go[torch.arange(nc), :, torch.arange(nc)] = 1
        grads = torch.autograd.grad(y, zs, grad_outputs=go, is_grads_batched=True, allow_unused=True)
    out = []
    for layer, z, g in zip(layers, zs, grads):
        if g is None:
            g = z.new_zeros((nc,) + tuple(z.shape))
        out.append((captured[layer][0], g.movedim(0, 1).contiguous()))
    return y.detach(), out


def conv_jacobian_rows(layer: torch.nn.Conv2d, a: Tensor, D: Tensor) -> Tensor:
    """A Conv2d layer's Jacobian rows (n, nc, nA*nG) in the posterior's order from its
    input a (n, C, H, W) and D (n, nc, Cout, Ho, Wo) of layer_io_jacobians:
    M_{b,c} = unfold(a_b) D_{b,c}^T, bias row sum_p D_{b,c}[:, p]."""
    unf = torch.nn.functional.unfold(a, layer.kernel_size, dilation=layer.dilation,
                                     padding=layer.padding, stride=layer.stride)  # (n, C*kh*kw, P)
    n, nc, nG = D.shape[:3]
    Dp = D.reshape(n, nc, nG, -1)
    M = torch.einsum("bkp,bcgp->bckg", unf, Dp)
    if layer.bias is not None:
        M = torch.cat([M, Dp.sum(-1).unsqueeze(2)], dim=2)
    return M.reshape(n, nc, -1)


def _conv_rows_uncovered(layer: torch.nn.Conv2d):
    """Why kfac_cov_conv_rows does not cover `layer` (None: it does)."""
    if tuple(layer.dilation) != (1, 1):
        return f"dilation {tuple(layer.dilation)}"
    if layer.groups != 1:
        return f"groups {layer.groups}"
    if layer.padding_mode != "zeros":
        return f"padding_mode {layer.padding_mode!r}"
    if isinstance(layer.padding, str):
        return f"padding {layer.padding!r}"
    return None


def conv_jacobian_rows_device(layer: torch.nn.Conv2d, a: Tensor, D: Tensor) -> Tensor:
    """conv_jacobian_rows by one device launch (kfac_cov_conv_rows): the im2col stays
    implicit, the classes share one GEMM per sample, the bias row is the ones column.
    a (n, C, H, W) and D (n, nc, Cout, Ho, Wo) fp32 on a HIP device; returns (n, nc, nA*nG)
    fp32 in the posterior's order.  a may be a batch view (sample stride >= C*H*W, the
    inner dimensions contiguous) and D may have padded rows (row stride >= nG*L): neither is
    copied; anything else is.  Two calls give identical bits and a row depends on its own
    a_b, D[b, c] only.  Raises ValueError for what the kernel does not cover: dilation != 1,
    groups != 1, padding_mode != "zeros", string padding."""
    why = _conv_rows_uncovered(layer)
    if why is not None:
        raise ValueError(f"conv_jacobian_rows_device does not cover {why}; use conv_jacobian_rows")
    a, D = a.detach(), D.detach()
    if a.dim() != 4 or D.dim() != 5 or D.shape[0] != a.shape[0]:
        raise ValueError(f"a {tuple(a.shape)} / D {tuple(D.shape)}: expected (n, C, H, W) and "
                         f"(n, nc, Cout, Ho, Wo)")
    N.require_device(a, "a", layer)
    N.require_device(D, "D", layer)
    n, C, H, W = a.shape
    nc, nG = D.shape[1], D.shape[2]
    if C != layer.in_channels or nG != layer.out_channels:
        raise ValueError(f"a {tuple(a.shape)} / D {tuple(D.shape)} do not fit {layer}")
    nA = C * layer.kernel_size[0] * layer.kernel_size[1] + (layer.bias is not None)
    M = torch.empty(n, nc, nA * nG, dtype=torch.float32, device=a.device)
    if n == 0 or nc == 0:
        return M
    if not a[0].is_contiguous() or (n > 1 and a.stride(0) < C * H * W):
        a = a.contiguous()
    op = N.patch_operand(a[:1], layer.kernel_size, layer.padding, layer.stride, layer.bias is not None)
    L = op.L
    if (D.shape[3], D.shape[4]) != (op.Ho, op.Wo):
        raise ValueError(f"D {tuple(D.shape)}: {layer} maps a {tuple(a.shape)} to {op.Ho} x {op.Wo} positions")
    if D[0, 0].is_contiguous():  # D[b, c] is one nG*L block: a view, whatever the outer strides
        D3 = D.as_strided((n, nc, nG * L), (D.stride(0), D.stride(1), 1))
    else:
        D3 = D.contiguous().view(n, nc, nG * L)
    D3, ldD = _cov_rows(D3, nG * L)
    op.rows = n * L
    op.sB = a.stride(0) if n > 1 else C * H * W
    N.cov_conv_rows([N.cov_conv_rows_job(op, D3, ldD, nG, M, nA * nG)], n, nc, a.device)
    return M


def _conv_rows(layer: torch.nn.Conv2d, a: Tensor, D: Tensor) -> Tensor:
    """The factored route's Conv2d rows: on the device where kfac_cov_conv_rows covers the
    layer, from torch (conv_jacobian_rows) where it does not."""
    if _conv_rows_uncovered(layer) is None:
        return conv_jacobian_rows_device(layer, a, D)
    return conv_jacobian_rows(layer, a, D)


def _cov_outer_jobs(terms, lower: bool, who: str, max_classes: int = None):
    """(tensors to keep alive, kfac_cov_outer_job tuples, nb, nc) of [(a_l, D_l, K1_l, K2_l)]."""
    return _kron_jobs(terms, True, lower, who, max_classes)


def _cov_outer_job_at(j, b0: int, nc: int):
    """The kfac_cov_outer_job tuple j with a and D starting at sample b0."""
    return (j[0] + 4 * b0 * j[1], j[1], j[2], j[3], j[4] + 4 * b0 * nc * j[5], *j[5:])


def kron_covariance_outer(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]], lower: bool = True,
                          max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance for Linear layers without their Jacobian rows:
    cov[b] = sum_l ||K1_l^T abar_l[b]||^2 (D_l[b] K2_l)(D_l[b] K2_l)^T, abar = [a | 1].

    terms: [(a_l, D_l, K1_l, K2_l)] as layer_io_jacobians returns them: a (nb, cols) the
    layer's input, D (nb, nc, nG) or (nc, nG), K1 (nA x nA) with nA = cols + 1 (bias: the
    ones column is implicit) or nA = cols, K2 (nG x nG); `lower` marks K1 / K2
    lower-triangular.  Returns (nb, nc, nc) fp32, every block bitwise symmetric.  More
    than 8 terms fold in groups of 8; the samples are cut into chunks that need at most
    `max_workspace_bytes` of scratch each (a sample's block depends on that sample only,
    so chunking does not change a bit).
    """
    keep, jobs, nb, nc = _cov_outer_jobs(terms, lower, "kron_covariance_outer", MAX_COV_CLASSES)
    return _run_per_sample(jobs, N.CovOuterJob, _cov_outer_job_at, N.kron_cov_outer_workspace_bytes,
                           N.kron_cov_outer, nb, nc, keep[0].device, max_workspace_bytes)


def kron_covariance_outer_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]], lower: bool = True,
                                max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_outer for any number of outputs: the same terms, the same (nb, nc, nc)
    fp32 result, nc not capped (kfac_kron_cov_outer_tiled).  A 512 -> 1000 head costs its
    V = D K2 (nb*1000 x 1000) and the Gram partials, never a Jacobian row.

    Every block is bitwise symmetric, two calls give identical bits, terms fold in groups of
    8 and the samples are chunked under `max_workspace_bytes` without changing a bit, as in
    kron_covariance_outer; against it (nc <= 32, another summation order) the result agrees
    to fp32 rounding.
    """
    keep, jobs, nb, nc = _cov_outer_jobs(terms, lower, "kron_covariance_outer_tiled")
    return _run_per_sample(jobs, N.CovOuterJob, _cov_outer_job_at, N.kron_cov_outer_tiled_workspace_bytes,
                           N.kron_cov_outer_tiled, nb, nc, keep[0].device, max_workspace_bytes)


def _per_sample_calls(nc: int):
    """(dense, outer) per-sample covariance calls for nc outputs: the 32x32-quadrant kernels
    up to MAX_COV_CLASSES, the class-tiled ones above."""
    if nc > MAX_COV_CLASSES:
        return kron_covariance_tiled, kron_covariance_outer_tiled
    return kron_covariance, kron_covariance_outer


def _glm_chunk_factored(model, layers, inv, x):
    """One chunk of the factored route: Linear layers by kron_covariance_outer, Conv2d
    layers by kron_covariance on rows formed from the same captures (_conv_rows: on the
    device for every layer kfac_cov_conv_rows covers); the two are added.  More than
    MAX_COV_CLASSES outputs go through the class-tiled calls (_per_sample_calls)."""
    f, io = layer_io_jacobians(model, layers, x)
    outer, dense = [], []
    for layer, (a, D) in zip(layers, io):
        if isinstance(layer, torch.nn.Linear):
            if a.dim() != 2:
                raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
            outer.append((a, D, *inv[layer]))
        elif isinstance(layer, torch.nn.Conv2d):
            dense.append((_conv_rows(layer, a, D), *inv[layer]))
        else:
            raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                             f"{layer.__class__.__name__}")
    cov_dense, cov_outer = _per_sample_calls(f.shape[1])
    cov = cov_outer(outer, lower=True) if outer else None
    if dense:
        conv = cov_dense(dense, lower=True)
        cov = conv if cov is None else cov + conv
    return f, cov


def _run_joint(jobs, struct, workspace_bytes, call, nb, nc, device, max_workspace_bytes):
    """What the two joint calls share: the (nb, nc, nb, nc) result, jobs folded in groups
    of 8 with `accumulate`, one call over all samples (cross blocks need both samples' rows,
    so nothing is chunked)."""
    out = torch.empty(nb * nc, nb * nc, dtype=torch.float32, device=device)
    if nb > 0:
        groups = [[struct(*j) for j in jobs[i:i + 8]] for i in range(0, len(jobs), 8)]
        need = max(workspace_bytes(g, nb, nc) for g in groups)
        if need == 0:
            raise ValueError(f"nb = {nb}, nc = {nc}: the joint covariance's {nb * nc} rows exceed one call")
        if need > max_workspace_bytes:
            raise ValueError(f"the joint call needs {need} workspace bytes, max_workspace_bytes is "
                             f"{max_workspace_bytes} (the samples of a joint covariance cannot be chunked)")
        for gi, g in enumerate(groups):
            call(g, nb, nc, out, accumulate=gi > 0)
    return out.view(nb, nc, nb, nc)


def kron_covariance_joint(terms: Sequence[Tuple[Tensor, Tensor, Tensor]], lower: bool = True,
                          max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance across the samples: cov[b, c, b', c'] =
    sum_l J_l[b, c] (K1_l K1_l^T kron K2_l K2_l^T) J_l[b', c']^T, the joint (function-space)
    covariance of all nb*nc outputs of the call.

    terms as kron_covariance takes them; nc has no cap here (for the per-sample blocks alone
    at any number of outputs use kron_covariance_tiled, which computes no cross block and
    has these diagonal blocks' bits).  Returns (nb, nc, nb, nc) fp32, a view of the
    contiguous (nb*nc x nb*nc) matrix, bitwise symmetric: cov[b, c, b', c'] == cov[b', c', b, c];
    its diagonal blocks cov[b, :, b, :] are kron_covariance's (marginal_blocks).  An entry
    depends on its two rows only, so the result for a subset of the samples has the bits of
    those sub-blocks.  More than 8 terms fold in groups of 8.  The samples cannot be
    chunked: a call that needs more than `max_workspace_bytes` of scratch raises ValueError.
    """
    keep, jobs, nb, nc = _cov_jobs(terms, lower, "kron_covariance_joint")
    return _run_joint(jobs, N.CovJob, N.kron_cov_joint_workspace_bytes, N.kron_cov_joint, nb, nc,
                      keep[0].device, max_workspace_bytes)


def kron_covariance_outer_joint(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]], lower: bool = True,
                                max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_joint for Linear layers without their Jacobian rows:
    cov[b, c, b', c'] = sum_l (U_l U_l^T)[b, b'] (V_l V_l^T)[(b, c), (b', c')] with
    U_l = [a_l | 1] K1_l (nb x nA) and V_l = D_l K2_l (nb*nc x nG).

    terms as kron_covariance_outer takes them; the scratch is U, V and the Gram partials,
    so a 4097 x 4096 layer is as cheap to hold as a small one.  Returns (nb, nc, nb, nc) fp32
    with kron_covariance_joint's guarantees (cov[b, c, b', c'] == cov[b', c', b, c] bitwise).
    """
    keep, jobs, nb, nc = _cov_outer_jobs(terms, lower, "kron_covariance_outer_joint")
    return _run_joint(jobs, N.CovOuterJob, N.kron_cov_outer_joint_workspace_bytes, N.kron_cov_outer_joint,
                      nb, nc, keep[0].device, max_workspace_bytes)


def marginal_blocks(cov: Tensor) -> Tensor:
    """The per-sample blocks cov[b, :, b, :] of a joint covariance (N, nc, N, nc) as
    (N, nc, nc), what glm_predictive(joint=False) returns and probit_predictive takes.
    Pure torch."""
    if cov.dim() != 4 or cov.shape[0] != cov.shape[2] or cov.shape[1] != cov.shape[3]:
        raise ValueError(f"cov {tuple(cov.shape)}: expected (N, nc, N, nc)")
    return torch.diagonal(cov, dim1=0, dim2=2).permute(2, 0, 1).contiguous()


def _glm_joint(model, layers, inv, x, chunk, jacobians):
    """glm_predictive(joint=True): Jacobians (dense) or captures (factored) chunk by chunk,
    concatenated along the samples, then one joint call per route."""
    logits, dense_rows, captures = [], [[] for _ in layers], [[] for _ in layers]
    for c0 in range(0, x.shape[0], chunk):
        xc = x[c0:c0 + chunk]
        if jacobians == "dense":
            f, Js = output_jacobians(model, layers, xc)
            for rows, J in zip(dense_rows, Js):
                rows.append(J)
        else:
            f, io = layer_io_jacobians(model, layers, xc)
            for li, (layer, (a, D)) in enumerate(zip(layers, io)):
                if isinstance(layer, torch.nn.Linear):
                    if a.dim() != 2:
                        raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
                    captures[li].append((a, D))
                elif isinstance(layer, torch.nn.Conv2d):
                    dense_rows[li].append(_conv_rows(layer, a, D))
                else:
                    raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                                     f"{layer.__class__.__name__}")
        logits.append(f)
    outer = [(torch.cat([a for a, _ in cap]), torch.cat([D for _, D in cap]), *inv[layer])
             for layer, cap in zip(layers, captures) if cap]
    dense = [(torch.cat(rows), *inv[layer]) for layer, rows in zip(layers, dense_rows) if rows]
    cov = kron_covariance_outer_joint(outer, lower=True) if outer else None
    if dense:
        rows = kron_covariance_joint(dense, lower=True)
        cov = rows if cov is None else cov + rows
    return torch.cat(logits), cov


def glm_predictive(kfac, x: Tensor, layers: Iterable = None, chunk: int = 64, jacobians: str = "dense",
                   joint: bool = False):
    """The linearised (GLM) predictive of `kfac.model` under the KFAC posterior
    (KFAC.invert's factors, the Gaussian KFAC.sample draws from): (logits (N, nc),
    cov (N, nc, nc)) with cov = sum_l J_l (L_A L_A^T kron L_G L_G^T) J_l^T, in chunks
    of `chunk` samples.  No sampling loop, no weight replacement; a regression net
    with one output has its predictive variance in cov[:, 0, 0].  Any number of outputs:
    up to MAX_COV_CLASSES = 32 a chunk goes through kron_covariance / kron_covariance_outer,
    above (a CIFAR-100 or ImageNet head) through kron_covariance_tiled /
    kron_covariance_outer_tiled, on either route.

    jacobians="dense" materialises every Jacobian row (output_jacobians); "factored"
    takes one layer_io_jacobians call per chunk and never forms a Linear layer's rows
    (kron_covariance_outer), which is what a wide layer needs; a Conv2d layer's rows come
    from the same captures in one device launch (conv_jacobian_rows_device).

    joint=True returns cov (N, nc, N, nc), the covariance across the samples too (the
    function-space posterior over x; cov[b, c, b', c'] == cov[b', c', b, c] bitwise): the
    Jacobians or captures are still taken `chunk` samples at a time, then ONE joint call
    covers all N (kron_covariance_joint / kron_covariance_outer_joint).  marginal_blocks
    gives the joint=False result back."""
    if jacobians not in ("dense", "factored"):
        raise ValueError(f"jacobians must be 'dense' or 'factored', got {jacobians!r}")
    model = kfac.model
    if layers is None:
        layers = [m for m in list(model.modules())[1:] if m in kfac.state]
    layers = list(layers)
    inv = kfac.inv_state
    if joint:
        return _glm_joint(model, layers, inv, x, chunk, jacobians)
    logits, covs = [], []
    for c0 in range(0, x.shape[0], chunk):
        if jacobians == "factored":
            f, cov = _glm_chunk_factored(model, layers, inv, x[c0:c0 + chunk])
            logits.append(f)
            covs.append(cov)
            continue
        f, Js = output_jacobians(model, layers, x[c0:c0 + chunk])
        logits.append(f)
        cov_dense, _ = _per_sample_calls(f.shape[1])
        covs.append(cov_dense([(J, *inv[layer]) for layer, J in zip(layers, Js)], lower=True))
    return torch.cat(logits), torch.cat(covs)


# ------------------------------------------------------------ damping sweeps
# A = V_A diag(lam_A) V_A^T (KFAC.eigh) gives KFAC.invert's L_A L_A^T = V_A diag(w_A) V_A^T with
# w_A = 1 / (sqrt(s) lam_A + sqrt(n)): in the eigenbasis a damping (add n, multiply s) is a
# pair of weight vectors, and a grid of dampings shares the forward pass, the Jacobians or
# captures and the projections on V_A / V_G (kfac_kron_cov_sweep, kfac_kron_cov_outer_sweep).
MAX_SWEEP = 64  # grid points per device call


def damping_weights(lam: Tensor, dampings: Sequence[Tuple[float, float]]) -> Tensor:
    """w[t, i] = 1 / (sqrt(s_t) lam[i] + sqrt(n_t)) for dampings [(add n_t, multiply s_t)]:
    (nt, n) fp32, computed in fp64 on lam's device.  Raises numpy.linalg.LinAlgError if a
    shifted eigenvalue is not positive (KFAC.invert's non-SPD condition).  Pure torch."""
    d = torch.tensor([[float(n), float(s)] for n, s in dampings], dtype=torch.float64,
                     device=lam.device).reshape(-1, 2)
    r = d[:, 1:2].sqrt() * lam.detach().to(torch.float64).reshape(1, -1) + d[:, 0:1].sqrt()
    if not bool((r > 0).all()):
        raise np.linalg.LinAlgError("damping_weights: sqrt(multiply) * eigenvalue + sqrt(add) is not "
                                    "positive (the damped factor is not positive definite)")
    return r.reciprocal().to(torch.float32)


def _damping_grid(dampings, count: int):
    """[[(add, multiply) per state entry] per grid point], each pair parsed as KFAC.invert
    parses its arguments (scalars, or two per-entry lists)."""
    from .curvatures import KFAC
    grid = [KFAC._damping(None, add, multiply, count) for add, multiply in dampings]
    if not grid:
        raise ValueError("no dampings")
    return grid


def _sweep_weight_rows(w: Tensor, n: int, what: str):
    """w as (nt, n): the shape check, which needs no device."""
    w = w.detach()
    if w.dim() == 1:
        w = w.unsqueeze(0)
    if w.dim() != 2 or w.shape[1] != n:
        raise ValueError(f"{what} {tuple(w.shape)}: expected (nt, {n})")
    return w


def _sweep_weights(w: Tensor, n: int, what: str):
    """(w (nt, n) of _sweep_weight_rows with unit column stride, its row stride)."""
    N.require_device(w, what)
    if w.stride(1) != 1 or (w.shape[0] > 1 and w.stride(0) < n):
        w = w.contiguous()
    return w, (w.stride(0) if w.shape[0] > 1 else n)


def _square(V: Tensor, what: str) -> int:
    """The order of a square matrix of eigenvectors: the shape check, which needs no device."""
    if V.dim() != 2 or V.shape[0] != V.shape[1]:
        raise ValueError(f"{what} {tuple(V.shape)}: expected a square matrix of eigenvectors")
    return V.shape[0]


def _sweep_basis(V: Tensor, what: str):
    """(V, square by _square, with unit column stride, its row stride)."""
    N.require_device(V, what)
    V = V.detach() if V.stride(-1) == 1 else V.detach().contiguous()
    return V, max(V.stride(0), V.shape[0])


def _run_sweep(build, workspace_bytes, call, njobs, nb, nc, nt, device, max_workspace_bytes):
    """The chunking the two sweeps share: `build(i, b0, t0)` is job i's struct for samples
    from b0 and grid points from t0.  Jobs fold in groups of 8, grid points go in calls of
    MAX_SWEEP, the samples in chunks that need at most `max_workspace_bytes` of scratch."""
    out = torch.empty(nt, nb, nc, nc, dtype=torch.float32, device=device)
    if nb == 0:
        return out
    groups = [range(i, min(i + 8, njobs)) for i in range(0, njobs, 8)]
    tmax = min(nt, MAX_SWEEP)

    def need(n):
        return max(workspace_bytes([build(i, 0, 0) for i in g], n, nc, tmax) for g in groups)

    step = nb
    while step > 1 and need(step) > max_workspace_bytes:
        step = max(1, min(step - 1, step * max_workspace_bytes // need(step)))
    if need(step) > max_workspace_bytes:
        raise ValueError(f"one sample needs {need(1)} workspace bytes, max_workspace_bytes is "
                         f"{max_workspace_bytes}")
    for t0 in range(0, nt, MAX_SWEEP):
        ntc = min(MAX_SWEEP, nt - t0)
        for b0 in range(0, nb, step):
            n = min(step, nb - b0)
            # a call writes (ntc, n, nc, nc) contiguously: a sample chunk goes through a copy
            dst = out[t0:t0 + ntc] if n == nb else torch.empty(ntc, n, nc, nc, dtype=torch.float32,
                                                               device=device)
            for gi, g in enumerate(groups):
                call([build(i, b0, t0) for i in g], n, nc, ntc, dst, accumulate=gi > 0)
            if n != nb:
                out[t0:t0 + ntc, b0:b0 + n] = dst
    return out


def _weighted(parse, struct, terms, outer: bool, who: str, max_classes, workspace_bytes, call,
              max_workspace_bytes):
    """What the eight weighted calls share: the terms parsed and checked by `parse`
    (_sweep_jobs / _full_jobs), then `call` through _run_sweep; `max_classes` None: no cap."""
    keep, jobs, nb, nc, nt = parse(terms, outer, who, max_classes)
    job_at = _cov_outer_job_at if outer else _cov_job_at

    def build(i, b0, t0):
        # the head moves to sample b0, the weights' (pointer, row stride) pairs to grid point t0
        fixed, weights = jobs[i]
        if len(weights) == 1:
            (W, ldW), = weights
            return struct(*job_at(fixed, b0, nc), W + 4 * t0 * ldW, ldW)
        (wA, ldwA), (wG, ldwG) = weights
        return struct(*job_at(fixed, b0, nc), wA + 4 * t0 * ldwA, ldwA, wG + 4 * t0 * ldwG, ldwG)

    return _run_sweep(build, workspace_bytes, call, len(jobs), nb, nc, nt, keep[0].device, max_workspace_bytes)


def _sweep_jobs(terms, outer: bool, who: str, max_classes):
    """(tensors to keep alive, per term (the job tuple up to ldG, [(wA, ldwA), (wG, ldwG)]), nb,
    nc, nt) of [(J_l, VA_l, VG_l, wA_l, wG_l)] or, outer, [(a_l, D_l, VA_l, VG_l, wA_l, wG_l)]."""
    def shapes(term):
        if outer:
            a, D, VA, VG, wA, wG = term
        else:
            J, VA, VG, wA, wG = term
        nA, nG = _square(VA, "VA"), _square(VG, "VG")
        head = _outer_head(a, D, nA, nG, "VA", VA) if outer else _rows_head(J, nA, nG)
        wA, wG = _sweep_weight_rows(wA, nA, "wA"), _sweep_weight_rows(wG, nG, "wG")
        return head, (VA, VG, wA, wG), (wA.shape[0], wG.shape[0])

    parsed, nb, nc, nt = _parse_terms(terms, shapes, who, max_classes, "rows")
    keep, jobs = [], []
    for head, (VA, VG, wA, wG) in parsed:
        VAc, ldA = _sweep_basis(VA, "VA")
        VGc, ldG = _sweep_basis(VG, "VG")
        if not outer:
            fields = head(keep)
        wAc, ldwA = _sweep_weights(wA, VAc.shape[0], "wA")
        wGc, ldwG = _sweep_weights(wG, VGc.shape[0], "wG")
        if outer:  # (a and D have always been looked at after the weights here)
            fields = head(keep)
        keep.extend([VAc, VGc, wAc, wGc])
        jobs.append(((*fields, VAc.data_ptr(), ldA, VGc.data_ptr(), ldG),
                     ((wAc.data_ptr(), ldwA), (wGc.data_ptr(), ldwG))))
    return keep, jobs, nb, nc, nt


def kron_covariance_sweep(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]],
                          max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance over a grid of nt weightings in the factors' eigenbasis:
    cov[t, b, c, c'] = sum_l sum_{i,g} wA_l[t, i] wG_l[t, g] Y_l[b, c][i, g] Y_l[b, c'][i, g],
    Y_l[b, c] = VA_l^T M_l[b, c] VG_l projected once for all t.

    terms: [(J_l, VA_l, VG_l, wA_l, wG_l)], J as kron_covariance takes it, VA (nA x nA) /
    VG (nG x nG) eigenvectors as columns, wA (nt, nA) / wG (nt, nG) non-negative weights
    (damping_weights).  Returns (nt, nb, nc, nc) fp32; per grid point kron_covariance's
    guarantees hold, and slice t has the bits of the call with row t's weights alone.  Shapes are
    checked (ValueError) before anything touches the device.
    """
    return _weighted(_sweep_jobs, N.CovSweepJob, terms, False, "kron_covariance_sweep", MAX_COV_CLASSES,
                     N.kron_cov_sweep_workspace_bytes, N.kron_cov_sweep, max_workspace_bytes)


def kron_covariance_sweep_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]],
                                max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_sweep for any number of outputs: the same terms, the same
    (nt, nb, nc, nc) fp32 result, nc not capped (kfac_kron_cov_sweep_tiled: a sample's block in
    64x64 class tiles, the weights folded into one operand as it is loaded).  The guarantees
    are kron_covariance_sweep's; with every weight 1 slice t has the bits of
    kron_covariance_tiled(lower=False) on the same rows; against kron_covariance_sweep
    (nc <= 32, another summation order) it agrees to fp32 rounding."""
    return _weighted(_sweep_jobs, N.CovSweepJob, terms, False, "kron_covariance_sweep_tiled", None,
                     N.kron_cov_sweep_tiled_workspace_bytes, N.kron_cov_sweep_tiled, max_workspace_bytes)


def kron_covariance_outer_sweep(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]],
                                max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_outer over a grid of nt weightings in the factors' eigenbasis:
    cov[t, b] = sum_l (sum_i wA_l[t, i] p_l[b][i]^2) Q_l[b] diag(wG_l[t]) Q_l[b]^T with
    p_l[b] = VA_l^T [a_l[b] | 1] and Q_l[b] = D_l[b] VG_l projected once for all t.

    terms: [(a_l, D_l, VA_l, VG_l, wA_l, wG_l)], a and D as kron_covariance_outer takes them,
    VA (nA x nA, nA = cols + 1 with the implicit ones column, or cols), VG (nG x nG), wA
    (nt, nA), wG (nt, nG).  Returns (nt, nb, nc, nc) fp32 with kron_covariance_sweep's
    guarantees.
    """
    return _weighted(_sweep_jobs, N.CovOuterSweepJob, terms, True, "kron_covariance_outer_sweep", MAX_COV_CLASSES,
                     N.kron_cov_outer_sweep_workspace_bytes, N.kron_cov_outer_sweep, max_workspace_bytes)


def kron_covariance_outer_sweep_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]],
                                      max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_outer_sweep for any number of outputs: the same terms, the same
    (nt, nb, nc, nc) fp32 result, nc not capped (kfac_kron_cov_outer_sweep_tiled).  The
    guarantees are kron_covariance_sweep's; against kron_covariance_outer_sweep (nc <= 32,
    another summation order) it agrees to fp32 rounding."""
    return _weighted(_sweep_jobs, N.CovOuterSweepJob, terms, True, "kron_covariance_outer_sweep_tiled", None,
                     N.kron_cov_outer_sweep_tiled_workspace_bytes, N.kron_cov_outer_sweep_tiled, max_workspace_bytes)


def _sweep_calls(nc: int):
    """(dense, outer) damping-sweep covariance calls for nc outputs, as _per_sample_calls."""
    if nc > MAX_COV_CLASSES:
        return kron_covariance_sweep_tiled, kron_covariance_outer_sweep_tiled
    return kron_covariance_sweep, kron_covariance_outer_sweep


def glm_predictive_sweep(kfac, x: Tensor, dampings, layers: Iterable = None, chunk: int = 64,
                         jacobians: str = "dense"):
    """glm_predictive for a grid of dampings from ONE eigendecomposition of the factors:
    (logits (N, nc), cov (nt, N, nc, nc)), cov[t] what `kfac.invert(*dampings[t])` followed by
    glm_predictive gives, without an inversion.  `dampings`: a sequence of (add, multiply),
    each a scalar pair or two per-layer lists as KFAC.invert takes them.  The forward pass,
    the Jacobians (or captures) and the projections on the eigenvectors are shared by the
    grid; each grid point costs one weighted contraction.  Uses `kfac.eig_state`, calling
    `kfac.eigh()` when nothing is cached.  `jacobians` as in glm_predictive: "factored" sends
    Linear layers through kron_covariance_outer_sweep and Conv2d layers through
    kron_covariance_sweep on their rows (conv_jacobian_rows_device where the kernel covers the
    layer, conv_jacobian_rows otherwise)."""
    if jacobians not in ("dense", "factored"):
        raise ValueError(f"jacobians must be 'dense' or 'factored', got {jacobians!r}")
    model = kfac.model
    entries = list(kfac.state)
    if layers is None:
        layers = [m for m in list(model.modules())[1:] if m in kfac.state]
    layers = list(layers)
    grid = _damping_grid(dampings, len(entries))
    eig = kfac.eig_state or kfac.eigh()
    basis = {}
    for layer in layers:
        (lamA, VA), (lamG, VG) = eig[layer]
        pairs = [point[entries.index(layer)] for point in grid]
        basis[layer] = (VA, VG, damping_weights(lamA, pairs), damping_weights(lamG, pairs))
    logits, covs = [], []
    for c0 in range(0, x.shape[0], chunk):
        xc = x[c0:c0 + chunk]
        if jacobians == "dense":
            f, Js = output_jacobians(model, layers, xc)
            cov_dense, _ = _sweep_calls(f.shape[1])
            cov = cov_dense([(J, *basis[layer]) for layer, J in zip(layers, Js)])
        else:
            f, io = layer_io_jacobians(model, layers, xc)
            outer, dense = [], []
            for layer, (a, D) in zip(layers, io):
                if isinstance(layer, torch.nn.Linear):
                    if a.dim() != 2:
                        raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
                    outer.append((a, D, *basis[layer]))
                elif isinstance(layer, torch.nn.Conv2d):
                    dense.append((_conv_rows(layer, a, D), *basis[layer]))
                else:
                    raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                                     f"{layer.__class__.__name__}")
            cov_dense, cov_outer = _sweep_calls(f.shape[1])
            cov = cov_outer(outer) if outer else None
            if dense:
                conv = cov_dense(dense)
                cov = conv if cov is None else cov + conv
        logits.append(f)
        covs.append(cov)
    return torch.cat(logits), torch.cat(covs, dim=1)


def log_det_sweep(eig_state, dampings) -> Tensor:
    """log det of the damped Kronecker curvature per grid point, from the eigenvalues:
    out[t] = sum_layers nG sum_i log(sqrt(s) lamA[i] + sqrt(n)) + nA sum_g log(sqrt(s) lamG[g] + sqrt(n))
           = -2 sum_layers (nG sum log diag L_A + nA sum log diag L_G)   of KFAC.invert's factors,
    the other half of an evidence-style criterion.  `eig_state`: KFAC.eigh's dictionary, or
    the KFAC object (its cached eigenpairs, else eigh()).  Returns (nt,) fp64.  Pure torch."""
    if not isinstance(eig_state, dict):
        eig_state = eig_state.eig_state or eig_state.eigh()
    entries = list(eig_state.values())
    grid = _damping_grid(dampings, len(entries))
    lam0 = entries[0][0][0]
    out = torch.zeros(len(grid), dtype=torch.float64, device=lam0.device)
    for index, ((lamA, _), (lamG, _)) in enumerate(entries):
        d = torch.tensor([[float(point[index][0]), float(point[index][1])] for point in grid],
                         dtype=torch.float64, device=lam0.device)
        terms = []
        for lam in (lamA, lamG):
            r = d[:, 1:2].sqrt() * lam.detach().to(torch.float64).reshape(1, -1) + d[:, 0:1].sqrt()
            if not bool((r > 0).all()):
                raise np.linalg.LinAlgError("log_det_sweep: sqrt(multiply) * eigenvalue + sqrt(add) is "
                                            "not positive (the damped factor is not positive definite)")
            terms.append(r.log().sum(dim=1))
        out += lamG.numel() * terms[0] + lamA.numel() * terms[1]
    return out


# ------------------------------------------------- per-entry eigenbasis weights (EFB)
# EFB keeps the KFAC eigenbases and refits every one of the nA*nG eigenvalues: EFB.sample draws
# S = V_A (Z o Lambda^-T) V_G^T with Lambda^- = inv_state (nG x nA) = (s lam + n)^(-1/2), so
# cov = sum_layers sum_{i,g} W[i][g] Y[i][g] Y'[i][g] with W = (Lambda^-)^T squared: the sweep
# calls' contraction with an arbitrary weight per (i, g) (kfac_kron_cov_full,
# kfac_kron_cov_outer_full).  A damping grid costs no inversion and no eigendecomposition.
def _full_shapes(VA: Tensor, VG: Tensor, W: Tensor):
    """(nA, nG, W as (nt, nA, nG)) after the shape checks, which need no device."""
    nA, nG = _square(VA, "VA"), _square(VG, "VG")
    W = W.detach()
    if W.dim() == 2:
        W = W.unsqueeze(0)
    if W.dim() != 3 or tuple(W.shape[1:]) != (nA, nG):
        raise ValueError(f"W {tuple(W.shape)}: expected (nt, {nA}, {nG}) or ({nA}, {nG})")
    return nA, nG, W


def _full_weights(W: Tensor):
    """(W (nt, nA, nG) with its matrices contiguous blocks, the stride between them)."""
    N.require_device(W, "W")
    nt, nA, nG = W.shape
    if not W[0].is_contiguous() or (nt > 1 and W.stride(0) < nA * nG):
        W = W.contiguous()
    return W, (W.stride(0) if nt > 1 else nA * nG)


def _full_jobs(terms, outer: bool, who: str, max_classes):
    """(tensors to keep alive, per term (the job tuple up to ldG, [(W, ldW)]), nb, nc, nt) of
    [(J_l, VA_l, VG_l, W_l)] or, outer, [(a_l, D_l, VA_l, VG_l, W_l)]."""
    def shapes(term):
        if outer:
            a, D, VA, VG, W = term
        else:
            J, VA, VG, W = term
        nA, nG, W3 = _full_shapes(VA, VG, W)
        head = _outer_head(a, D, nA, nG, "VA", VA) if outer else _rows_head(J, nA, nG)
        return head, (VA, VG, W3), (W3.shape[0],)

    parsed, nb, nc, nt = _parse_terms(terms, shapes, who, max_classes, "matrices")
    keep, jobs = [], []
    for head, (VA, VG, W3) in parsed:
        VAc, ldA = _sweep_basis(VA, "VA")
        VGc, ldG = _sweep_basis(VG, "VG")
        fields = head(keep)
        Wc, ldW = _full_weights(W3)
        keep.extend([VAc, VGc, Wc])
        jobs.append(((*fields, VAc.data_ptr(), ldA, VGc.data_ptr(), ldG), ((Wc.data_ptr(), ldW),)))
    return keep, jobs, nb, nc, nt


def kron_covariance_full(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]],
                         max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_sweep with a weight per eigenbasis entry instead of a rank-one pair:
    cov[t, b, c, c'] = sum_l sum_{i,g} W_l[t, i, g] Y_l[b, c][i, g] Y_l[b, c'][i, g],
    Y_l[b, c] = VA_l^T M_l[b, c] VG_l projected once for all t.

    terms: [(J_l, VA_l, VG_l, W_l)], J, VA, VG as kron_covariance_sweep takes them, W
    (nt, nA, nG) or (nA, nG) non-negative (efb_weights).  Returns (nt, nb, nc, nc) fp32 with
    kron_covariance_sweep's guarantees: bitwise symmetric blocks, a sample's block depends on
    that sample only, slice t has the bits of the call with W[t] alone.  Shapes are checked
    (ValueError) before anything touches the device.
    """
    return _weighted(_full_jobs, N.CovFullJob, terms, False, "kron_covariance_full", MAX_COV_CLASSES,
                     N.kron_cov_full_workspace_bytes, N.kron_cov_full, max_workspace_bytes)


def kron_covariance_full_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]],
                               max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_full for any number of outputs: the same terms, the same
    (nt, nb, nc, nc) fp32 result, nc not capped (kfac_kron_cov_full_tiled: a sample's block in
    64x64 class tiles, the weights folded into one operand as it is loaded).  The guarantees
    are kron_covariance_full's; with every weight 1 slice t has the bits of
    kron_covariance_tiled(lower=False) on the same rows; against kron_covariance_full
    (nc <= 32, another summation order) it agrees to fp32 rounding."""
    return _weighted(_full_jobs, N.CovFullJob, terms, False, "kron_covariance_full_tiled", None,
                     N.kron_cov_full_tiled_workspace_bytes, N.kron_cov_full_tiled, max_workspace_bytes)


def kron_covariance_outer_full(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]],
                               max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_full for Linear layers without their Jacobian rows:
    cov[t, b] = sum_l Q_l[b] diag(r_l[t, b]) Q_l[b]^T, r_l[t, b][g] = sum_i p_l[b][i]^2 W_l[t, i, g],
    with p_l[b] = VA_l^T [a_l[b] | 1] and Q_l[b] = D_l[b] VG_l projected once for all t.

    terms: [(a_l, D_l, VA_l, VG_l, W_l)], a, D, VA, VG as kron_covariance_outer_sweep takes
    them, W (nt, nA, nG) or (nA, nG).  Returns (nt, nb, nc, nc) fp32 with
    kron_covariance_full's guarantees.
    """
    return _weighted(_full_jobs, N.CovOuterFullJob, terms, True, "kron_covariance_outer_full", MAX_COV_CLASSES,
                     N.kron_cov_outer_full_workspace_bytes, N.kron_cov_outer_full, max_workspace_bytes)


def kron_covariance_outer_full_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]],
                                     max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_outer_full for any number of outputs: the same terms, the same
    (nt, nb, nc, nc) fp32 result, nc not capped (kfac_kron_cov_outer_full_tiled).  The
    guarantees are kron_covariance_full's; against kron_covariance_outer_full (nc <= 32,
    another summation order) it agrees to fp32 rounding."""
    return _weighted(_full_jobs, N.CovOuterFullJob, terms, True, "kron_covariance_outer_full_tiled", None,
                     N.kron_cov_outer_full_tiled_workspace_bytes, N.kron_cov_outer_full_tiled, max_workspace_bytes)


def _full_calls(nc: int):
    """(dense, outer) per-entry-weight covariance calls for nc outputs, as _per_sample_calls."""
    if nc > MAX_COV_CLASSES:
        return kron_covariance_full_tiled, kron_covariance_outer_full_tiled
    return kron_covariance_full, kron_covariance_outer_full


def efb_weights(lam: Tensor, dampings: Sequence[Tuple[float, float]]) -> Tensor:
    """W[t, i, g] = 1 / (s_t lam[g, i] + n_t) for dampings [(add n_t, multiply s_t)] and an EFB
    state entry lam (nG, nA): (nt, nA, nG) fp32, the TRANSPOSE of the state's layout (the
    posterior's order), EFB.invert's inv_state squared; EFB damps with s and n themselves, not
    their square roots.  Computed in fp64 on lam's device.  Raises numpy.linalg.LinAlgError
    if any s lam + n is not positive.  Pure torch."""
    if lam.dim() != 2:
        raise ValueError(f"lam {tuple(lam.shape)}: expected an EFB state entry (nG, nA)")
    d = torch.tensor([[float(n), float(s)] for n, s in dampings], dtype=torch.float64,
                     device=lam.device).reshape(-1, 2)
    r = d[:, 1].reshape(-1, 1, 1) * lam.detach().to(torch.float64).t().unsqueeze(0) + d[:, 0].reshape(-1, 1, 1)
    if not bool((r > 0).all()):
        raise np.linalg.LinAlgError("efb_weights: multiply * eigenvalue + add is not positive")
    return r.reciprocal().to(torch.float32).contiguous()


def _efb_layers(efb, layers):
    if layers is None:
        layers = [m for m in list(efb.model.modules())[1:] if m in efb.state]
    return list(layers)


def _efb_chunk(model, layers, basis, x, jacobians):
    """(logits, cov (nt, n, nc, nc)) of one chunk; basis[layer] = (VA, VG, W (nt, nA, nG))."""
    if jacobians == "dense":
        f, Js = output_jacobians(model, layers, x)
        cov_dense, _ = _full_calls(f.shape[1])
        return f, cov_dense([(J, *basis[layer]) for layer, J in zip(layers, Js)])
    f, io = layer_io_jacobians(model, layers, x)
    outer, dense = [], []
    for layer, (a, D) in zip(layers, io):
        if isinstance(layer, torch.nn.Linear):
            if a.dim() != 2:
                raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
            outer.append((a, D, *basis[layer]))
        elif isinstance(layer, torch.nn.Conv2d):
            dense.append((_conv_rows(layer, a, D), *basis[layer]))
        else:
            raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                             f"{layer.__class__.__name__}")
    cov_dense, cov_outer = _full_calls(f.shape[1])
    cov = cov_outer(outer) if outer else None
    if dense:
        conv = cov_dense(dense)
        cov = conv if cov is None else cov + conv
    return f, cov


def glm_predictive_efb(efb, x: Tensor, layers: Iterable = None, chunk: int = 64, jacobians: str = "dense"):
    """glm_predictive under the EFB posterior (EFB.invert's inv_state, the Gaussian EFB.sample
    draws from): (logits (N, nc), cov (N, nc, nc)) with
    cov = sum_l sum_{i,g} W_l[i][g] Y_l[i][g] Y_l'[i][g], Y = V_A^T M V_G, W = inv_state^T squared,
    in chunks of `chunk` samples: no sampling loop, no weight replacement.  `jacobians` as in
    glm_predictive: "dense" sends output_jacobians' rows through kron_covariance_full;
    "factored" sends Linear layers through kron_covariance_outer_full and Conv2d layers through
    kron_covariance_full on rows formed from the same captures."""
    if jacobians not in ("dense", "factored"):
        raise ValueError(f"jacobians must be 'dense' or 'factored', got {jacobians!r}")
    assert efb.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
    layers = _efb_layers(efb, layers)
    basis = {layer: (*efb.eigvecs[layer], (efb.inv_state[layer].detach().t() ** 2).contiguous().unsqueeze(0))
             for layer in layers}
    logits, covs = [], []
    for c0 in range(0, x.shape[0], chunk):
        f, cov = _efb_chunk(efb.model, layers, basis, x[c0:c0 + chunk], jacobians)
        logits.append(f)
        covs.append(cov[0])
    return torch.cat(logits), torch.cat(covs)


def glm_predictive_efb_sweep(efb, x: Tensor, dampings, layers: Iterable = None, chunk: int = 64,
                             jacobians: str = "dense", max_weight_bytes: int = 1 << 30) -> Tensor:
    """glm_predictive_efb's covariance for a grid of dampings straight from `efb.state`:
    cov (nt, N, nc, nc), cov[t] what `efb.invert(*dampings[t])` followed by glm_predictive_efb
    gives.  No invert call is needed (EFB.invert is elementwise: a grid point is a weight
    matrix, efb_weights).  `dampings`: a sequence of (add, multiply), each a scalar pair or two
    per-layer lists.  The weights are built for as many grid points at a time as fit in
    `max_weight_bytes` over all layers (a 4097 x 4096 layer's matrix is 67 MB per grid point);
    within such a group the forward pass, the Jacobians or captures and the projections are
    shared."""
    if jacobians not in ("dense", "factored"):
        raise ValueError(f"jacobians must be 'dense' or 'factored', got {jacobians!r}")
    assert efb.state, "State dict is empty. Did you call 'update' prior to this?"
    entries = list(efb.state)
    layers = _efb_layers(efb, layers)
    grid = _damping_grid(dampings, len(entries))
    per_point = sum(4 * efb.state[layer].numel() for layer in layers)
    group = max(1, min(len(grid), max_weight_bytes // max(per_point, 1)))
    out = []
    for t0 in range(0, len(grid), group):
        points = grid[t0:t0 + group]
        basis = {layer: (*efb.eigvecs[layer],
                         efb_weights(efb.state[layer], [p[entries.index(layer)] for p in points]))
                 for layer in layers}
        covs = [_efb_chunk(efb.model, layers, basis, x[c0:c0 + chunk], jacobians)[1]
                for c0 in range(0, x.shape[0], chunk)]
        out.append(torch.cat(covs, dim=1))
        del basis
    return torch.cat(out)


def efb_log_det_sweep(efb, dampings) -> Tensor:
    """log det of the damped EFB curvature per grid point: out[t] = sum_layers sum log(s lam + n)
    over every entry of `efb.state`, the other half of an evidence-style criterion (as
    log_det_sweep is for KFAC).  Returns (nt,) fp64.  Raises numpy.linalg.LinAlgError if any
    s lam + n is not positive.  Pure torch."""
    assert efb.state, "State dict is empty. Did you call 'update' prior to this?"
    entries = list(efb.state.values())
    grid = _damping_grid(dampings, len(entries))
    out = torch.zeros(len(grid), dtype=torch.float64, device=entries[0].device)
    for index, lam in enumerate(entries):
        d = torch.tensor([[float(point[index][0]), float(point[index][1])] for point in grid],
                         dtype=torch.float64, device=lam.device)
        r = d[:, 1:2] * lam.detach().to(torch.float64).reshape(1, -1) + d[:, 0:1]
        if not bool((r > 0).all()):
            raise np.linalg.LinAlgError("efb_log_det_sweep: multiply * eigenvalue + add is not positive")
        out += r.log().sum(dim=1)
    return out


# ------------------------------------------------------------ GLM predictive under the INF posterior
# INF's posterior is Gaussian with precision P = s (U Lambda U^T + D+) + n I, U = kron(U_A, U_G)
# (nA*nG x r), D+ the diagonal correction clipped at 0.  By Woodbury, with w = 1 / (s D+ + n),
# sigma = sqrt(s Lambda), B = chol(I + sigma U^T diag(w) U sigma) and F = B^-1 diag(sigma):
#   P^-1 = diag(w) - diag(w) U F^T F U^T diag(w) ,
# so cov = (W-weighted Gram of the rows) - (Gram of F t), t = U_A^T (M o W) U_G
# (kfac_inf_cov, kfac_inf_cov_outer): the posterior INF defines, exactly, with no square root
# of the covariance and no sampling loop.  INF.sample (the reference's sampler, ported
# literally) is left as it is.
def _inf_shapes(UA: Tensor, UG: Tensor, W: Tensor, F: Tensor):
    """(nA, nG, ra, rg) after the shape checks, which need no device."""
    for U, what in ((UA, "UA"), (UG, "UG")):
        if U.dim() != 2 or U.shape[0] == 0 or U.shape[1] == 0:
            raise ValueError(f"{what} {tuple(U.shape)}: expected a (n, rank) matrix of eigenvectors")
    (nA, ra), (nG, rg) = UA.shape, UG.shape
    if tuple(W.shape) != (nA, nG):
        raise ValueError(f"W {tuple(W.shape)}: expected ({nA}, {nG})")
    if tuple(F.shape) != (ra * rg, ra * rg):
        raise ValueError(f"F {tuple(F.shape)}: expected ({ra * rg}, {ra * rg})")
    return nA, nG, ra, rg


def _inf_operands(UA: Tensor, UG: Tensor, W: Tensor, F: Tensor):
    """(tensors to keep alive, the job tuple's last ten fields UA, ldA, ra, ..., F, ldF)."""
    for t, what in ((UA, "UA"), (UG, "UG"), (W, "W"), (F, "F")):
        N.require_device(t, what)
    # (a view goes through uncopied only if its rows have unit stride and lie at least their
    # width apart: an expanded tensor's row stride 0 is not a leading dimension)
    UA, UG, F = (t.detach() if t.stride(-1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1])
                 else t.detach().contiguous() for t in (UA, UG, F))
    W = W.detach().contiguous()
    ld = lambda t: max(t.stride(0), t.shape[1])  # noqa: E731
    return [UA, UG, W, F], (UA.data_ptr(), ld(UA), UA.shape[1], UG.data_ptr(), ld(UG), UG.shape[1],
                            W.data_ptr(), W.numel(), F.data_ptr(), ld(F))


def _inf_jobs(terms, outer: bool, who: str, max_classes):
    """_inf_dense_jobs (outer False) / _inf_outer_jobs (outer True)."""
    def shapes(term):
        if outer:
            a, D, UA, UG, W, F = term
        else:
            J, UA, UG, W, F = term
        nA, nG, _, _ = _inf_shapes(UA, UG, W, F)
        return (_outer_head(a, D, nA, nG, "UA", UA) if outer else _rows_head(J, nA, nG)), (UA, UG, W, F), ()

    parsed, nb, nc, _ = _parse_terms(terms, shapes, who, max_classes)
    keep, jobs = [], []
    for head, operands in parsed:
        fields = head(keep)
        held, tail = _inf_operands(*operands)
        keep.extend(held)
        jobs.append((*fields, *tail))
    return keep, jobs, nb, nc


def _inf_dense_jobs(terms, who, max_classes):
    """(tensors to keep alive, kfac_inf_cov_job tuples, nb, nc) of [(J_l, UA_l, UG_l, W_l, F_l)]
    (max_classes None: no cap)."""
    return _inf_jobs(terms, False, who, max_classes)


def _inf_dense(terms, who, max_classes, workspace_bytes, call, max_workspace_bytes):
    """kron_covariance_inf / kron_covariance_inf_tiled: the terms parsed and checked, then
    `call` per sample chunk."""
    keep, jobs, nb, nc = _inf_dense_jobs(terms, who, max_classes)
    return _run_per_sample(jobs, N.InfCovJob, _cov_job_at, workspace_bytes, call, nb, nc, keep[0].device,
                           max_workspace_bytes)


def kron_covariance_inf(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]],
                        max_workspace_bytes: int = 1 << 30) -> Tensor:
    """cov[b, c, c'] = sum_l [ sum_{i,g} W_l[i, g] M_l[b, c][i, g] M_l[b, c'][i, g]
                               - < F_l t_l[b, c], F_l t_l[b, c'] > ],
    t_l[b, c] = UA_l^T (M_l[b, c] o W_l) UG_l flattened p*rg + q: J P^-1 J^T under the INF
    posterior (inf_covariance_factors).

    terms: [(J_l, UA_l, UG_l, W_l, F_l)], J (nb, nc, nA*nG) or (nc, nA*nG) in the posterior's
    order (posterior_jacobian), UA (nA, ra), UG (nG, rg), W (nA, nG) non-negative, F (ra*rg,
    ra*rg).  Returns (nb, nc, nc) fp32: every block bitwise symmetric, a sample's block depends
    on that sample only (chunking under `max_workspace_bytes` changes no bit), two calls give
    identical bits, more than 8 terms fold in groups of 8.  The diagonal is a difference of two
    non-negative sums and is not clamped: it may come out negative at rounding level.  Shapes
    are checked (ValueError) before anything touches the device.  At most MAX_COV_CLASSES
    outputs: kron_covariance_inf_tiled has no cap.
    """
    return _inf_dense(terms, "kron_covariance_inf", MAX_COV_CLASSES, N.inf_cov_workspace_bytes, N.inf_cov,
                      max_workspace_bytes)


def kron_covariance_inf_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]],
                              max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_inf for any number of outputs (a CIFAR-100 or ImageNet head): the same
    terms, the same shape checks before anything touches the device, the same (nb, nc, nc)
    fp32 result, nc not capped (kfac_inf_cov_tiled: a sample's block in 64x64 class tiles, the
    weighted Gram of the raw rows and the Gram of F t kept as separate fp32 partials whose
    difference is formed in fp64).

    Every block is bitwise symmetric; two calls give identical bits; a sample's block depends
    on that sample only, so chunking under `max_workspace_bytes` changes no bit; padded strides
    of J, UA, UG and F change no bit; terms fold in groups of 8; the diagonal is not clamped.
    With F = 0 the result has the bits of kron_covariance_full_tiled on the same J and W with
    identity VA, VG.  Against kron_covariance_inf (nc <= 32, another segmentation) it agrees to
    fp32 rounding only.
    """
    return _inf_dense(terms, "kron_covariance_inf_tiled", None, N.inf_cov_tiled_workspace_bytes,
                      N.inf_cov_tiled, max_workspace_bytes)


def _inf_outer_jobs(terms, who, max_classes):
    """(tensors to keep alive, kfac_inf_cov_outer_job tuples, nb, nc) of
    [(a_l, D_l, UA_l, UG_l, W_l, F_l)] (max_classes None: no cap)."""
    return _inf_jobs(terms, True, who, max_classes)


def _inf_outer(terms, who, max_classes, workspace_bytes, call, max_workspace_bytes):
    """kron_covariance_outer_inf / kron_covariance_outer_inf_tiled: the terms parsed and
    checked, then `call` per sample chunk."""
    keep, jobs, nb, nc = _inf_outer_jobs(terms, who, max_classes)
    return _run_per_sample(jobs, N.InfCovOuterJob, _cov_outer_job_at, workspace_bytes, call, nb, nc,
                           keep[0].device, max_workspace_bytes)


def kron_covariance_outer_inf(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]],
                              max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_inf for Linear layers without their Jacobian rows (M[b, c] =
    [a[b] | 1] D[b, c]^T): cov[b] = sum_l [ D_l[b] diag(rho_l[b]) D_l[b]^T - Y_l[b] Y_l[b]^T ],
    rho[b][g] = sum_i abar[b][i]^2 W[i, g], Y[b][c] = F t[b, c],
    t[b, c][p, q] = sum_g H[b][p, g] D[b, c][g] UG[g, q], H[b][p, g] = sum_i UA[i, p] abar[b][i] W[i, g].

    terms: [(a_l, D_l, UA_l, UG_l, W_l, F_l)], a (nb, cols) and D (nb, nc, nG) as
    layer_io_jacobians returns them, UA (nA, ra) with nA = cols + 1 (bias: the ones column is
    implicit) or nA = cols, UG, W, F as in kron_covariance_inf, whose guarantees hold.  At most
    MAX_COV_CLASSES outputs: kron_covariance_outer_inf_tiled has no cap.
    """
    return _inf_outer(terms, "kron_covariance_outer_inf", MAX_COV_CLASSES, N.inf_cov_outer_workspace_bytes,
                      N.inf_cov_outer, max_workspace_bytes)


def kron_covariance_outer_inf_tiled(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]],
                                    max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_covariance_outer_inf for any number of outputs: the same terms and shape checks, nc
    not capped (kfac_inf_cov_outer_tiled: 64x64 class tiles of D_b diag(rho_b) D_b^T on the raw
    D rows and of Y_b Y_b^T, separate fp32 partials whose difference is formed in fp64).

    kron_covariance_inf_tiled's guarantees hold: bitwise symmetric blocks, identical bits from
    two calls, a sample's block depends on that sample only (chunking changes no bit), padded
    strides of a, D, UA, UG and F change no bit, the diagonal is not clamped.  Against
    kron_covariance_outer_inf (nc <= 32) and against kron_covariance_inf_tiled on the
    materialised rows it agrees to fp32 rounding only.
    """
    return _inf_outer(terms, "kron_covariance_outer_inf_tiled", None, N.inf_cov_outer_tiled_workspace_bytes,
                      N.inf_cov_outer_tiled, max_workspace_bytes)


def _inf_calls(nc: int):
    """(dense call, factored call) of the INF covariance for nc outputs: the capped calls up to
    MAX_COV_CLASSES, the class-tiled ones above."""
    if nc > MAX_COV_CLASSES:
        return kron_covariance_inf_tiled, kron_covariance_outer_inf_tiled
    return kron_covariance_inf, kron_covariance_outer_inf


def _inf_layer_factors(inf, add, multiply, layers):
    """[(layer, UA, UG, d = s D+ + n (nA, nG) fp64, sigma = sqrt(s Lambda), B^-1)] from
    `inf.state`, B = chol(I + sigma U^T diag(1/d) U sigma); inf.state is only read."""
    from .curvatures import INF, KFAC
    assert inf.state, "State dict is empty. Did you call 'update' prior to this?"
    entries = list(inf.state)
    damping = KFAC._damping(None, add, multiply, len(entries))
    out = []
    for layer in (entries if layers is None else list(layers)):
        n, s = damping[entries.index(layer)]
        UA, UG, lam, correction = inf.state[layer]
        d = float(s) * correction.detach().to(torch.float64).clamp(min=0.0) + float(n)
        if not bool((d > 0).all()):
            raise np.linalg.LinAlgError("INF: multiply * correction + add is not positive")
        sigma = (s * lam.detach()).sqrt()
        c = d.reciprocal().sqrt().to(torch.float32)
        vtv = N.kron_gram(UA.detach(), UG.detach(), c, sigma)
        (B_inv,) = INF._chol_inverse((vtv + vtv.t()) / 2., (1.0,))
        out.append((layer, UA.detach(), UG.detach(), d.reshape(UA.shape[0], UG.shape[0]), sigma, B_inv))
    return out


def inf_covariance_factors(inf, add=0., multiply=1., layers: Iterable = None):
    """{layer: (UA, UG, W, F)} for kron_covariance_inf / kron_covariance_outer_inf from
    `inf.state` (INF.update's (U_A, U_G, Lambda, D)): W = 1 / (s D+ + n) as (nA, nG) fp32,
    computed in fp64 on the device, F = B^-1 diag(sigma) with sigma = sqrt(s Lambda) and
    B = chol(I + sigma U^T diag(w) U sigma) (N.kron_gram, INF._chol_inverse).  `add` / `multiply`
    are scalars or per-layer lists, as in INF.invert; no invert call is needed and `inf.state`
    is not modified (INF.invert clips the correction in place; this does not).  Raises
    numpy.linalg.LinAlgError where s D+ + n is not positive."""
    return {layer: (UA, UG, d.reciprocal().to(torch.float32).contiguous(), (B_inv * sigma[None, :]).contiguous())
            for layer, UA, UG, d, sigma, B_inv in _inf_layer_factors(inf, add, multiply, layers)}


def inf_draw_factors(inf, add=0., multiply=1., layers: Iterable = None):
    """{layer: (UA, UG, W, F, C, Binv)} for kron_draws_inf / kron_draws_outer_inf and
    inf_posterior_sample: inf_covariance_factors' (UA, UG, W, F), C = sqrt(W) = 1 / sqrt(s D+ + n)
    formed in fp64 and rounded to fp32 once, and Binv = B^-1 (r, r).  `add` / `multiply` as in
    inf_covariance_factors; `inf.state` is only read."""
    return {layer: (UA, UG, d.reciprocal().to(torch.float32).contiguous(), (B_inv * sigma[None, :]).contiguous(),
                    d.reciprocal().sqrt().to(torch.float32).contiguous(), B_inv.contiguous())
            for layer, UA, UG, d, sigma, B_inv in _inf_layer_factors(inf, add, multiply, layers)}


def inf_posterior_sample(UA: Tensor, UG: Tensor, W: Tensor, F: Tensor, C: Tensor, Binv: Tensor, z: Tensor,
                         e: Tensor) -> Tensor:
    """Weight draws x (ns, nA, nG) ~ N(0, P^-1) of one layer's INF posterior, exactly:
        x = C o z - W o [ UA mat(F^T q) UG^T ] ,   q = F vec(UA^T (C o z) UG) + Binv e ,
    (UA, UG, W, F, C, Binv) from inf_draw_factors, z (ns, nA, nG) and e (ns, r) standard normal
    and independent (Matheron's rule on P^-1 = diag(w) - diag(w) U F^T F U^T diag(w); without
    the e part the covariance lacks a term).  x[s] is in the posterior's (nA, nG) layout: the
    layer's weight moves by x[s, :cols].T and its bias by x[s, cols].  Plain torch, any device
    and dtype: the sample the logit draws of kron_draws_inf correspond to, and what INF.sample
    (the reference's sampler, ported literally) is not."""
    ns, (ra, rg) = z.shape[0], (UA.shape[1], UG.shape[1])
    cz = C * z
    g = (UA.t() @ cz @ UG).reshape(ns, ra * rg)
    q = g @ F.t() + e @ Binv.t()
    return cz - W * (UA @ (q @ F).reshape(ns, ra, rg) @ UG.t())


def inf_log_det(inf, add=0., multiply=1.) -> Tensor:
    """log det of the INF precision P = s (U Lambda U^T + D+) + n I over every layer of
    `inf.state`: sum_layers [ sum log(s D+ + n) - 2 sum log diag(B^-1) ] (0-dim fp64), the
    counterpart of log_det_sweep / efb_log_det_sweep."""
    total = None
    for _, _, _, d, _, B_inv in _inf_layer_factors(inf, add, multiply, None):
        term = d.log().sum() - 2.0 * B_inv.diagonal().to(torch.float64).log().sum()
        total = term if total is None else total + term
    return total


def _inf_chunk(model, layers, factors, x, jacobians):
    """(logits, cov (n, nc, nc)) of one chunk; factors[layer] = (UA, UG, W, F).  More than
    MAX_COV_CLASSES outputs go through the class-tiled calls (_inf_calls)."""
    if jacobians == "dense":
        f, Js = output_jacobians(model, layers, x)
        return f, _inf_calls(f.shape[1])[0]([(J, *factors[layer]) for layer, J in zip(layers, Js)])
    f, io = layer_io_jacobians(model, layers, x)
    outer, dense = [], []
    for layer, (a, D) in zip(layers, io):
        if isinstance(layer, torch.nn.Linear):
            if a.dim() != 2:
                raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
            outer.append((a, D, *factors[layer]))
        elif isinstance(layer, torch.nn.Conv2d):
            dense.append((_conv_rows(layer, a, D), *factors[layer]))
        else:
            raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                             f"{layer.__class__.__name__}")
    cov_dense, cov_outer = _inf_calls(f.shape[1])
    cov = cov_outer(outer) if outer else None
    if dense:
        conv = cov_dense(dense)
        cov = conv if cov is None else cov + conv
    return f, cov


def glm_predictive_inf(inf, x: Tensor, add=0., multiply=1., layers: Iterable = None, chunk: int = 64,
                       jacobians: str = "dense"):
    """glm_predictive under the INF posterior, straight from `inf.state` (no invert call):
    (logits (N, nc), cov (N, nc, nc)), cov = sum_l J_l P_l^-1 J_l^T with P_l the precision
    s (U Lambda U^T + D+) + n I of layer l, in closed form (inf_covariance_factors), in chunks
    of `chunk` samples.  `jacobians` as in glm_predictive_efb: "dense" sends output_jacobians'
    rows through kron_covariance_inf; "factored" sends Linear layers through
    kron_covariance_outer_inf and Conv2d layers through kron_covariance_inf on rows formed from
    the same captures.  Any number of outputs: up to MAX_COV_CLASSES = 32 a chunk goes through
    these capped calls, above through kron_covariance_inf_tiled / kron_covariance_outer_inf_tiled
    (64x64 class tiles; bitwise symmetric blocks, chunking changes no bit)."""
    if jacobians not in ("dense", "factored"):
        raise ValueError(f"jacobians must be 'dense' or 'factored', got {jacobians!r}")
    layers = _efb_layers(inf, layers)
    factors = inf_covariance_factors(inf, add, multiply, layers)
    logits, covs = [], []
    for c0 in range(0, x.shape[0], chunk):
        f, cov = _inf_chunk(inf.model, layers, factors, x[c0:c0 + chunk], jacobians)
        logits.append(f)
        covs.append(cov)
    return torch.cat(logits), torch.cat(covs)


# ------------------------------------------------------------ Monte-Carlo GLM predictive
# A weight draw S = K1 Z K2^T moves the linearised logits by < T_r, Z >_F, T_r = K1^T M_r K2
# (kfac_glm_draws / kfac_glm_draws_outer): joint draws of the logits of all inputs, with
# glm_predictive(joint=True)'s covariance, without a weight sample or a forward pass per draw.
def _draw_z(z: Tensor, nA: int, nG: int, ns, index: int):
    """(z as (ns, nA, nG) with each draw one contiguous block, its draw stride)."""
    z = z.detach()
    if z.dim() != 3 or tuple(z.shape[1:]) != (nA, nG) or (ns is not None and z.shape[0] != ns):
        raise ValueError(f"z[{index}] {tuple(z.shape)}: expected ({'ns' if ns is None else ns}, {nA}, {nG})")
    N.require_device(z, f"z[{index}]")
    if z.shape[0] == 0:
        raise ValueError("no draws")
    if z.stride(2) != 1 or (nA > 1 and z.stride(1) != nG) or (z.shape[0] > 1 and z.stride(0) < nA * nG):
        z = z.contiguous()
    return z, (z.stride(0) if z.shape[0] > 1 else nA * nG)


def _z_at(zl, s0: int):
    """The draw fields (Z, ldZ) of a kfac_draw_job from draw s0 on; zl = (z, ldz)."""
    z, ldz = zl
    return z.data_ptr() + 4 * s0 * ldz, ldz


def _run_draws(jobs, zs, struct, rows_struct, job_at, workspace_bytes, call, nb, nc, device,
               max_workspace_bytes, draw_at=_z_at):
    """What the draw calls share: the (ns, nb, nc) result, jobs folded in groups of 8 with
    `accumulate`, the draws and then the samples halved until a call's scratch fits
    `max_workspace_bytes` (F[s][r] depends on draw s and row r only: no bit changes).
    `draw_at(zs[l], s0)`: the job struct's fields after `rows`, from draw s0 on."""
    ns = zs[0][0].shape[0]
    R = nb * nc
    out = torch.empty(ns, R, dtype=torch.float32, device=device)
    if nb == 0:
        return out.view(ns, nb, nc)
    groups = [list(zip(jobs[i:i + 8], zs[i:i + 8])) for i in range(0, len(jobs), 8)]

    def build(g, b0, s0):
        return [struct(rows_struct(*job_at(j, b0, nc)), *draw_at(zl, s0)) for j, zl in g]

    def need(n, m):
        return max(workspace_bytes(build(g, 0, 0), n, nc, m) for g in groups)

    bstep, sstep = nb, ns
    while need(bstep, sstep) > max_workspace_bytes:
        if sstep > 1:
            sstep = (sstep + 1) // 2
        elif bstep > 1:
            bstep = (bstep + 1) // 2
        else:
            raise ValueError(f"one sample and one draw need {need(1, 1)} workspace bytes, "
                             f"max_workspace_bytes is {max_workspace_bytes}")
    if need(bstep, sstep) == 0:
        raise ValueError(f"nb = {nb}, nc = {nc}, ns = {ns}: sizes beyond one call")
    for b0 in range(0, nb, bstep):
        n = min(bstep, nb - b0)
        for s0 in range(0, ns, sstep):
            m = min(sstep, ns - s0)
            for gi, g in enumerate(groups):
                call(build(g, b0, s0), n, nc, m, out[s0:s0 + m, b0 * nc:(b0 + n) * nc], accumulate=gi > 0)
    return out.view(ns, nb, nc)


def kron_draws(terms: Sequence[Tuple[Tensor, Tensor, Tensor]], z: Sequence[Tensor], lower: bool = True,
               max_workspace_bytes: int = 1 << 30) -> Tensor:
    """Logit draws from Jacobian rows: F[s, b, c] = sum_l < J_l[b, c] , K1_l z_l[s] K2_l^T >_F, what
    the weight draw K1 z K2^T (KFAC.sample's, from the same z) does to the linearised outputs.

    terms as kron_covariance_joint takes them; z[l] (ns, nA_l, nG_l) fp32, one standard-normal
    matrix per draw and term in the sampler's layout (a slice along the draws is used in
    place).  Returns (ns, nb, nc) fp32.  Two calls give identical bits, and F[s, b, c] depends
    on sample b's rows and draw s only, so subsets of the samples or of the draws reproduce
    their entries bit for bit.  More than 8 terms fold in groups of 8; the draws, then the
    samples, are cut until a call's scratch fits `max_workspace_bytes`.
    """
    keep, jobs, nb, nc = _cov_jobs(terms, lower, "kron_draws")
    if len(z) != len(jobs):
        raise ValueError(f"{len(jobs)} terms, {len(z)} draw tensors")
    zs = [_draw_z(zl, j[2], j[3], None if i == 0 else z[0].shape[0], i) for i, (zl, j) in enumerate(zip(z, jobs))]
    return _run_draws(jobs, zs, N.DrawJob, N.CovJob, _cov_job_at, N.glm_draws_workspace_bytes, N.glm_draws,
                      nb, nc, keep[0].device, max_workspace_bytes)


def kron_draws_outer(terms: Sequence[Tuple[Tensor, Tensor, Tensor, Tensor]], z: Sequence[Tensor],
                     lower: bool = True, max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_draws for Linear layers without their Jacobian rows:
    F[s, b, c] = sum_l u_l[b]^T z_l[s] v_l[b, c], U = [a | 1] K1 and V = D K2 as in
    kron_covariance_outer_joint.  Per draw 2 nb nA nG flops and one pass over z_l[s] per 64
    samples; no weight sample, no forward pass.

    terms as kron_covariance_outer_joint takes them, z and the guarantees as in kron_draws.
    """
    keep, jobs, nb, nc = _cov_outer_jobs(terms, lower, "kron_draws_outer")
    if len(z) != len(jobs):
        raise ValueError(f"{len(jobs)} terms, {len(z)} draw tensors")
    zs = [_draw_z(zl, j[2] + j[3], j[6], None if i == 0 else z[0].shape[0], i)
          for i, (zl, j) in enumerate(zip(z, jobs))]
    return _run_draws(jobs, zs, N.DrawOuterJob, N.CovOuterJob, _cov_outer_job_at,
                      N.glm_draws_outer_workspace_bytes, N.glm_draws_outer, nb, nc, keep[0].device,
                      max_workspace_bytes)


# Under the INF posterior a weight draw is x = C o Z - W o [UA mat(F^T q) UG^T],
# q = F vec(UA^T (C o Z) UG) + Binv eps (inf_posterior_sample), which moves the linearised logits
# by < M_r o C, Z > - < y_r, q >, y_r = F t_r the covariance calls' projection (kfac_inf_draws,
# kfac_inf_draws_outer).
def _inf_draw_at(zl, s0: int):
    """The fields (C, Binv, ldB, Z, ldZ, E, ldE) of a kfac_inf_draw_job from draw s0 on."""
    z, ldz, e, lde, C, Binv, ldB = zl
    return C.data_ptr(), Binv.data_ptr(), ldB, z.data_ptr() + 4 * s0 * ldz, ldz, e.data_ptr() + 4 * s0 * lde, lde


def _inf_draw_operands(terms, z, e, who):
    """(covariance terms, per-term (z, ldz, e, lde, C, Binv, ldB)) after the shape checks of C,
    Binv, z and e (ValueError before anything touches the device)."""
    terms = list(terms)
    if not terms:
        raise ValueError(f"{who}: no terms")
    if len(z) != len(terms) or len(e) != len(terms):
        raise ValueError(f"{who}: {len(terms)} terms, {len(z)} z and {len(e)} e draw tensors")
    cov_terms, shapes = [], []
    for *head, UA, UG, W, F, C, Binv in terms:
        nA, nG, ra, rg = _inf_shapes(UA, UG, W, F)
        r = ra * rg
        if tuple(C.shape) != (nA, nG):
            raise ValueError(f"C {tuple(C.shape)}: expected ({nA}, {nG})")
        if tuple(Binv.shape) != (r, r):
            raise ValueError(f"Binv {tuple(Binv.shape)}: expected ({r}, {r})")
        cov_terms.append((*head, UA, UG, W, F))
        shapes.append((nA, nG, r))
    ns = z[0].shape[0] if z[0].dim() == 3 else None
    for i, (el, (_, _, r)) in enumerate(zip(e, shapes)):
        if el.dim() != 2 or el.shape[1] != r or (ns is not None and el.shape[0] != ns):
            raise ValueError(f"e[{i}] {tuple(el.shape)}: expected ({'ns' if ns is None else ns}, {r})")
    zs = []
    for i, (zl, el, term, (nA, nG, r)) in enumerate(zip(z, e, terms, shapes)):
        zc, ldz = _draw_z(zl, nA, nG, ns, i)
        el = el.detach()
        N.require_device(el, f"e[{i}]")
        if el.stride(1) != 1 or (el.shape[0] > 1 and el.stride(0) < r):
            el = el.contiguous()
        C, Binv = term[-2].detach().contiguous(), term[-1].detach()
        N.require_device(C, "C")
        N.require_device(Binv, "Binv")
        if Binv.stride(1) != 1 or (r > 1 and Binv.stride(0) < r):
            Binv = Binv.contiguous()
        zs.append((zc, ldz, el, el.stride(0) if el.shape[0] > 1 else r, C, Binv, max(Binv.stride(0), r)))
    return cov_terms, zs


def kron_draws_inf(terms: Sequence[Tuple[Tensor, ...]], z: Sequence[Tensor], e: Sequence[Tensor],
                   max_workspace_bytes: int = 1 << 30) -> Tensor:
    """Logit draws under the INF posterior from Jacobian rows:
    F[s, b, c] = sum_l [ < J_l[b, c] o C_l , z_l[s] > - < F_l t_l[b, c] , q_l[s] > ],
    q_l[s] = F_l vec(UA_l^T (C_l o z_l[s]) UG_l) + Binv_l e_l[s], t as in kron_covariance_inf: what
    the weight draw inf_posterior_sample(..., z_l[s], e_l[s]) does to the linearised outputs.

    terms: [(J_l, UA_l, UG_l, W_l, F_l, C_l, Binv_l)], J as in kron_covariance_inf, the rest from
    inf_draw_factors; z[l] (ns, nA_l, nG_l) and e[l] (ns, ra_l*rg_l) fp32 standard normal (a slice
    along the draws is used in place).  Returns (ns, nb, nc) fp32, any nc.  Two calls give
    identical bits, and F[s, b, c] depends on sample b's rows and draw s only, so subsets of the
    samples or of the draws reproduce their entries bit for bit.  More than 8 terms fold in
    groups of 8; the draws, then the samples, are cut until a call's scratch fits
    `max_workspace_bytes`.  Shapes are checked (ValueError) before anything touches the device.
    """
    cov_terms, zs = _inf_draw_operands(terms, z, e, "kron_draws_inf")
    keep, jobs, nb, nc = _inf_dense_jobs(cov_terms, "kron_draws_inf", None)
    return _run_draws(jobs, zs, N.InfDrawJob, N.InfCovJob, _cov_job_at, N.inf_draws_workspace_bytes, N.inf_draws,
                      nb, nc, keep[0].device, max_workspace_bytes, _inf_draw_at)


def kron_draws_outer_inf(terms: Sequence[Tuple[Tensor, ...]], z: Sequence[Tensor], e: Sequence[Tensor],
                         max_workspace_bytes: int = 1 << 30) -> Tensor:
    """kron_draws_inf for Linear layers without their Jacobian rows (M[b, c] = [a[b] | 1] D[b, c]^T):
    F[s, b, c] = sum_l [ abar_l[b]^T (C_l o z_l[s]) D_l[b, c] - < F_l t_l[b, c] , q_l[s] > ].  Per
    draw 2 nb nA nG flops and one pass over z_l[s] and C_l per 64 samples, plus the projection
    of the draw itself (2 ra nA nG flops); no weight sample, no forward pass.

    terms: [(a_l, D_l, UA_l, UG_l, W_l, F_l, C_l, Binv_l)], a and D as in
    kron_covariance_outer_inf; z, e and the guarantees as in kron_draws_inf.  With F = 0 and
    Binv = 0 the result has the bits of kron_draws_outer on the same a, D with identity factors
    and z pre-multiplied by C in fp32.
    """
    cov_terms, zs = _inf_draw_operands(terms, z, e, "kron_draws_outer_inf")
    keep, jobs, nb, nc = _inf_outer_jobs(cov_terms, "kron_draws_outer_inf", None)
    return _run_draws(jobs, zs, N.InfDrawOuterJob, N.InfCovOuterJob, _cov_outer_job_at,
                      N.inf_draws_outer_workspace_bytes, N.inf_draws_outer, nb, nc, keep[0].device,
                      max_workspace_bytes, _inf_draw_at)


def _softmax_mc_finish(psum: Tensor, hsum: Tensor, ns: int):
    """(probs, expected_entropy, entropy, mutual_information) fp32 from the fp64 sums."""
    probs = psum / ns
    expected = hsum / ns
    entropy = torch.special.entr(probs).sum(dim=1)
    mi = (entropy - expected).clamp_min(0.0)
    return tuple(t.to(torch.float32) for t in (probs, expected, entropy, mi))


def softmax_mc_stats(logits: Tensor, draws: Tensor):
    """Monte-Carlo softmax statistics of logits (N, nc) + draws (S, N, nc) by kfac_softmax_mc:
    (probs (N, nc), expected_entropy (N,), entropy (N,), mutual_information (N,)), fp32.
    probs = mean_s softmax(logits + draws[s]); expected_entropy = mean_s H(softmax(.)) in nats;
    entropy = H(probs); mutual_information = entropy - expected_entropy (the epistemic part),
    finalised in fp64 from the device's fp64 sums and clamped at 0."""
    ns, nb, nc = draws.shape
    psum = torch.empty(nb, nc, dtype=torch.float64, device=logits.device)
    hsum = torch.empty(nb, dtype=torch.float64, device=logits.device)
    N.softmax_mc(logits.detach(), draws.detach(), psum, hsum)
    return _softmax_mc_finish(psum, hsum, ns)


class GLMPredictiveMC(NamedTuple):
    logits: Tensor
    probs: Tensor
    entropy: Tensor
    expected_entropy: Tensor
    mutual_information: Tensor
    draws: Optional[Tensor]


def glm_predictive_mc(curv, x: Tensor, n_draws: int = 100, layers: Iterable = None, chunk: int = 64,
                      jacobians: str = "factored", generator: torch.Generator = None,
                      z: Sequence[Tensor] = None, max_draw_bytes: int = 1 << 30,
                      return_draws: bool = False, add=0., multiply=1.) -> GLMPredictiveMC:
    """The Monte-Carlo GLM predictive of `curv.model`: `n_draws` posterior weight draws applied to
    the linearised network at every x, and the softmax statistics of the resulting logits --
    what `n_draws` x (sample_and_replace() + a forward pass) gives for a network that is linear
    in its weights, without a weight sample or a forward pass per draw.

    Returns (logits (N, nc), probs (N, nc), entropy (N,), expected_entropy (N,),
    mutual_information (N,), draws): softmax_mc_stats' quantities; `draws` is the
    (n_draws, N, nc) logit perturbations when `return_draws`, else None (they then exist one
    (draw chunk, sample chunk) block at a time).  Draw s is ONE weight sample applied to every
    x (the draws are jointly consistent across the inputs; their covariance is
    glm_predictive(joint=True)'s).  A regression net (nc = 1) has its use in `draws`; its
    statistics are the degenerate probs = 1, entropies 0.

    curv: a KFAC (factors inv_state, lower-triangular) or an EFB (K1 = V_A, K2 = V_G dense,
    z scaled elementwise by inv_state^T, as EFB.sample draws).  Routes as in glm_predictive:
    "factored" sends Linear layers through kron_draws_outer and Conv2d rows (_conv_rows) through
    kron_draws; "dense" sends output_jacobians' rows through kron_draws.

    The standard-normal z are drawn per draw chunk, for the layers in `layers` order (default:
    model.modules() order), each as torch.randn(chunk_draws, nA, nG, generator=generator) on the
    model's device; an explicit `z` -- a list of per-layer (n_draws, nA, nG) tensors in that
    order -- replaces them and is sliced, not copied (EFB: scaled into a new tensor).  A draw
    chunk holds as many draws as keep the live z within `max_draw_bytes`.  The samples go
    through `chunk` at a time inside each draw chunk, so with more than one draw chunk the
    captures (or Jacobians) of a sample chunk are recomputed per draw chunk; the generator is
    never replayed.  Chunking either way changes no bit of a draw.

    curv may also be an INF: no invert call is needed, the factors come from `inf.state` once per
    call (inf_draw_factors with `add` / `multiply`, which only INF uses, as glm_predictive_inf
    takes them), and the draws are exact draws of the INF posterior (inf_posterior_sample's;
    INF.sample's are not).  "factored" sends Linear layers through kron_draws_outer_inf and Conv2d
    rows through kron_draws_inf, "dense" output_jacobians' rows through kron_draws_inf.  Per draw
    chunk and for the layers in order, torch.randn(m, nA, nG, generator=...) and then
    torch.randn(m, r, generator=...), r the layer's rank; an explicit `z` is a list of per-layer
    (Z (n_draws, nA, nG), E (n_draws, r)) pairs, sliced and not copied; `max_draw_bytes` counts
    both."""
    if jacobians not in ("dense", "factored"):
        raise ValueError(f"jacobians must be 'dense' or 'factored', got {jacobians!r}")
    if n_draws < 1:
        raise ValueError(f"n_draws must be at least 1, got {n_draws}")
    from .curvatures import INF
    if isinstance(curv, INF):
        return _glm_mc_inf(curv, x, n_draws, layers, chunk, jacobians, generator, z, max_draw_bytes, return_draws,
                           add, multiply)
    assert curv.inv_state, "Inverse state dict is empty. Did you call 'invert' prior to this?"
    model = curv.model
    efb = hasattr(curv, "eigvecs")
    if layers is None:
        layers = [m for m in list(model.modules())[1:] if m in curv.state]
    layers = list(layers)
    factors = {layer: tuple(curv.eigvecs[layer] if efb else curv.inv_state[layer]) for layer in layers}
    shapes = [(factors[layer][0].shape[0], factors[layer][1].shape[0]) for layer in layers]
    if z is not None:
        z = list(z)
        if len(z) != len(layers):
            raise ValueError(f"{len(layers)} layers, {len(z)} draw tensors")
        for i, (zl, (nA, nG)) in enumerate(zip(z, shapes)):
            if tuple(zl.shape) != (n_draws, nA, nG):
                raise ValueError(f"z[{i}] {tuple(zl.shape)}: expected ({n_draws}, {nA}, {nG})")
    per_draw = 4 * sum(nA * nG for nA, nG in shapes)
    step = max(1, min(n_draws, max_draw_bytes // max(per_draw, 1)))
    N_, device = x.shape[0], factors[layers[0]][0].device
    logits, draws, psum, hsum = [], None, None, None
    for s0 in range(0, n_draws, step):
        m = min(step, n_draws - s0)
        if z is None:
            zc = [torch.randn(m, nA, nG, generator=generator, device=device, dtype=torch.float32)
                  for nA, nG in shapes]
            if efb:
                for zl, layer in zip(zc, layers):
                    zl *= curv.inv_state[layer].detach().t()
        else:
            zc = [zl[s0:s0 + m] for zl in z]
            if efb:
                zc = [zl * curv.inv_state[layer].detach().t() for zl, layer in zip(zc, layers)]
        for c0 in range(0, N_, chunk):
            xc = x[c0:c0 + chunk]
            outer, dense, zo, zd = [], [], [], []
            if jacobians == "dense":
                f, Js = output_jacobians(model, layers, xc)
                dense = [(J, *factors[layer]) for layer, J in zip(layers, Js)]
                zd = zc
            else:
                f, io = layer_io_jacobians(model, layers, xc)
                for layer, (a, D), zl in zip(layers, io, zc):
                    if isinstance(layer, torch.nn.Linear):
                        if a.dim() != 2:
                            raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
                        outer.append((a, D, *factors[layer]))
                        zo.append(zl)
                    elif isinstance(layer, torch.nn.Conv2d):
                        dense.append((_conv_rows(layer, a, D), *factors[layer]))
                        zd.append(zl)
                    else:
                        raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                                         f"{layer.__class__.__name__}")
            F = kron_draws_outer(outer, zo, lower=not efb) if outer else None
            if dense:
                rows = kron_draws(dense, zd, lower=not efb)
                F = rows if F is None else F + rows
            n, nc = f.shape
            if psum is None:
                psum = torch.empty(N_, nc, dtype=torch.float64, device=device)
                hsum = torch.empty(N_, dtype=torch.float64, device=device)
                if return_draws:
                    draws = torch.empty(n_draws, N_, nc, dtype=torch.float32, device=device)
            if s0 == 0:
                logits.append(f)
            N.softmax_mc(f.contiguous(), F, psum[c0:c0 + n], hsum[c0:c0 + n], accumulate=s0 > 0)
            if return_draws:
                draws[s0:s0 + m, c0:c0 + n] = F
        del zc
    if psum is None:  # no samples
        raise ValueError("x holds no samples")
    stats = _softmax_mc_finish(psum, hsum, n_draws)
    return GLMPredictiveMC(torch.cat(logits), stats[0], stats[2], stats[1], stats[3], draws)


def _glm_mc_inf(inf, x, n_draws, layers, chunk, jacobians, generator, z, max_draw_bytes, return_draws, add,
                multiply):
    """glm_predictive_mc under an INF posterior (arguments checked there)."""
    assert inf.state, "State dict is empty. Did you call 'update' prior to this?"
    model = inf.model
    layers = _efb_layers(inf, layers)
    shapes = []
    for layer in layers:
        UA, UG = inf.state[layer][0], inf.state[layer][1]
        shapes.append((UA.shape[0], UG.shape[0], UA.shape[1] * UG.shape[1]))
    if z is not None:
        z = [tuple(pair) for pair in z]
        if len(z) != len(layers):
            raise ValueError(f"{len(layers)} layers, {len(z)} (Z, E) draw pairs")
        for i, (pair, (nA, nG, r)) in enumerate(zip(z, shapes)):
            if len(pair) != 2 or tuple(pair[0].shape) != (n_draws, nA, nG) or tuple(pair[1].shape) != (n_draws, r):
                got = tuple(tuple(t.shape) for t in pair)
                raise ValueError(f"z[{i}] {got}: expected a pair ({n_draws}, {nA}, {nG}), ({n_draws}, {r})")
    factors = inf_draw_factors(inf, add, multiply, layers)
    per_draw = 4 * sum(nA * nG + r for nA, nG, r in shapes)
    step = max(1, min(n_draws, max_draw_bytes // max(per_draw, 1)))
    N_, device = x.shape[0], factors[layers[0]][0].device
    logits, draws, psum, hsum = [], None, None, None
    for s0 in range(0, n_draws, step):
        m = min(step, n_draws - s0)
        if z is None:
            zc = []
            for nA, nG, r in shapes:
                zl = torch.randn(m, nA, nG, generator=generator, device=device, dtype=torch.float32)
                zc.append((zl, torch.randn(m, r, generator=generator, device=device, dtype=torch.float32)))
        else:
            zc = [(zl[s0:s0 + m], el[s0:s0 + m]) for zl, el in z]
        for c0 in range(0, N_, chunk):
            xc = x[c0:c0 + chunk]
            outer, dense, zo, zd = [], [], [], []
            if jacobians == "dense":
                f, Js = output_jacobians(model, layers, xc)
                dense = [(J, *factors[layer]) for layer, J in zip(layers, Js)]
                zd = zc
            else:
                f, io = layer_io_jacobians(model, layers, xc)
                for layer, (a, D), zl in zip(layers, io, zc):
                    if isinstance(layer, torch.nn.Linear):
                        if a.dim() != 2:
                            raise ValueError(f"the factored route needs 2-D Linear inputs, got {tuple(a.shape)}")
                        outer.append((a, D, *factors[layer]))
                        zo.append(zl)
                    elif isinstance(layer, torch.nn.Conv2d):
                        dense.append((_conv_rows(layer, a, D), *factors[layer]))
                        zd.append(zl)
                    else:
                        raise ValueError(f"the factored route handles Linear and Conv2d layers, got "
                                         f"{layer.__class__.__name__}")
            F = kron_draws_outer_inf(outer, [p[0] for p in zo], [p[1] for p in zo]) if outer else None
            if dense:
                rows = kron_draws_inf(dense, [p[0] for p in zd], [p[1] for p in zd])
                F = rows if F is None else F + rows
            n, nc = f.shape
            if psum is None:
                psum = torch.empty(N_, nc, dtype=torch.float64, device=device)
                hsum = torch.empty(N_, dtype=torch.float64, device=device)
                if return_draws:
                    draws = torch.empty(n_draws, N_, nc, dtype=torch.float32, device=device)
            if s0 == 0:
                logits.append(f)
            N.softmax_mc(f.contiguous(), F, psum[c0:c0 + n], hsum[c0:c0 + n], accumulate=s0 > 0)
            if return_draws:
                draws[s0:s0 + m, c0:c0 + n] = F
        del zc
    if psum is None:  # no samples
        raise ValueError("x holds no samples")
    stats = _softmax_mc_finish(psum, hsum, n_draws)
    return GLMPredictiveMC(torch.cat(logits), stats[0], stats[2], stats[1], stats[3], draws)


def probit_predictive(logits: Tensor, cov: Tensor) -> Tensor:
    """softmax(logits / sqrt(1 + pi/8 * diag(cov))): the probit approximation of
    E[softmax(f)] for f ~ N(logits, cov).  Pure torch."""
    var = torch.diagonal(cov, dim1=-2, dim2=-1)
    return torch.softmax(logits / torch.sqrt(1.0 + (math.pi / 8.0) * var), dim=-1)


def argmax_grad_outputs(pred_mean: Tensor) -> Tensor:
    """grad_outputs[:, idx] = 1 with idx = argmax per row, set for EVERY row
    (classification_ll_block.py:119-121 semantics)."""
    idx = np.argmax(pred_mean.detach().cpu().numpy(), axis=1)
    grad_outputs = torch.zeros_like(pred_mean)
    grad_outputs[:, idx] = 1
    return grad_outputs


def entropy_bits(pred_std: float) -> float:
    """0.5 * log2(2 pi e var) (classification_ll_block.py:134-135)."""
    return float(0.5 * np.log2(2 * np.e * np.pi * pred_std))


def regression_inverse_factors(kfac, N_data: float, tau: float) -> List[Tuple[Tensor, Tensor]]:
    """pinv(N (q + tau I)) and pinv(N (h + tau I)) for every state entry
    (regression_ll_block.py:128-133).  q + tau I is SPD for tau > 0, so the
    pseudo-inverse is the inverse; computed by the fp64 device path."""
    jobs, outs = [], []
    device = None
    for layer, (q, h) in kfac.state.items():
        pair = []
        for F_ in (q, h):
            N.require_device(F_, "state", layer)
            out = torch.empty_like(F_, memory_format=torch.contiguous_format)
            jobs.append(N.invert_job(F_, out, float(N_data), float(N_data) * float(tau), N.OUT_INVERSE))
            pair.append(out)
            device = F_.device
        outs.append(tuple(pair))
    info = N.invert(jobs, device)
    if bool((info.cpu() != 0).any()):
        raise np.linalg.LinAlgError("SVD did not converge")
    return outs
