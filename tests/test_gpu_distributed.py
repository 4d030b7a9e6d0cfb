"""GPU, data-parallel KFAC with the real HIP kernels (models/curvatures.py:359-363 summed
over ranks):

* world 2 on one device (gloo carries the collective; RCCL cannot put two ranks on
  one GPU): the sharded pass reproduces single-device KFAC -- same factors (ONE
  packed-lower-triangle all-reduce per pass) and the same inverse Cholesky factors --
  over two passes with an uneven last batch; at C4's per-rank shape (8,192 rows per
  rank of a 16,384-row global batch); and with the inversion sharded over the ranks
  (each inverts its factors, one all-gather of the packed L triangles + verdicts);
* RCCL itself: a world-1 "nccl" process group running the same collectives
  (DistributedKFAC.always_reduce), so the RCCL all-reduce / all-gather path runs
  on the box;
* kfac_tri_pack / kfac_tri_unpack round trips, bit-exact.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

SIZES = {"small": ((512, 512, 300), 2), "c4": ((16384, 16384), 1)}  # global batches, passes


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _data(shape):
    rng = np.random.default_rng(7)
    out = []
    for gb in SIZES[shape][0]:
        out.append((rng.random((gb, 784), dtype=np.float32),
                    rng.standard_normal((gb, 128)).astype(np.float32),
                    rng.random((gb, 128), dtype=np.float32),
                    rng.standard_normal((gb, 10)).astype(np.float32)))
    return out


def _net(dev):
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(784, 128), torch.nn.ReLU(),
                               torch.nn.Linear(128, 10)).to(dev)


def _worker(rank, world, port, q, shape, shard, backend, launch_first=1, side=True, accumulate=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world))
    # RCCL: one rank per GPU; gloo: every rank on device 0 (one-GPU boxes)
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bnn_kfac_amd.distributed import DistributedKFAC
        net = _net(dev)
        kfac = DistributedKFAC(net, shard_inversion=shard)
        kfac.always_reduce = True
        kfac.launch_first = launch_first  # (16: the bench's pipelined loop, a pass per launch)
        kfac.side_collective = side  # the pass's collective on the inversion's side stream
        passes = 2 if accumulate else SIZES[shape][1]
        for p in range(passes):
            # accumulate: update, invert, update, invert with no reset() in between --
            # the second pass adds into the reduced state a side-stream collective
            # unpacked and an inversion read (the caller's stream must wait)
            if p == 0 or not accumulate:
                kfac.reset()
            for a1, g1, a2, g2 in _data(shape):
                gb = a1.shape[0]
                cut = [0, gb // 2 + (37 if shape == "small" else 0), gb][rank:rank + 2] if world == 2 \
                    else [0, gb]
                sl = slice(*cut)
                kfac.record[net[0]] = [torch.from_numpy(a1[sl]).to(dev), torch.from_numpy(g1[sl]).to(dev)]
                kfac.record[net[2]] = [torch.from_numpy(a2[sl]).to(dev), torch.from_numpy(g2[sl]).to(dev)]
                kfac.update(cut[1] - cut[0], global_batch_size=gb)
            kfac.invert(0.04, 200)
        st = [t.cpu().numpy() for pair in kfac.state.values() for t in pair]
        inv = [t.cpu().numpy() for pair in kfac.inv_state.values() for t in pair]
        q.put((rank, st, inv, kfac._sharded_last, kfac.side_collectives))
    finally:
        dist.destroy_process_group()


def _single_device(dev, shape, passes=1):
    from bnn_kfac_amd.curvatures import KFAC
    net = _net(dev)
    kfac = KFAC(net)
    for _ in range(passes):
        for a1, g1, a2, g2 in _data(shape):
            kfac.record[net[0]] = [torch.from_numpy(a1).to(dev), torch.from_numpy(g1).to(dev)]
            kfac.record[net[2]] = [torch.from_numpy(a2).to(dev), torch.from_numpy(g2).to(dev)]
            kfac.update(a1.shape[0])
    kfac.invert(0.04, 200)
    return ([t.cpu().numpy() for pair in kfac.state.values() for t in pair],
            [t.cpu().numpy() for pair in kfac.inv_state.values() for t in pair])


def _run(world, shape, shard, backend="gloo", launch_first=1, side=True, accumulate=False):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, shape, shard, backend, launch_first, side,
                                               accumulate))
             for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return results


def _check(results, want_st, want_inv, shard, side=True, expect_side=False):
    for rank, st, inv, sharded, side_passes in results:
        assert sharded == bool(shard)
        # the pass's collective ran on the inversion's side stream only when allowed
        # (replicated inversion); in the bench's shape (one launch per pass) it did
        if not side or shard:
            assert side_passes == 0, side_passes
        if expect_side:
            assert side_passes > 0, side_passes
        for g, w in zip(st, want_st):
            np.testing.assert_allclose(g, w, rtol=1e-5, atol=1e-5 * np.abs(w).max())
        # the reduced factors differ from the single-device sums in the last bits,
        # which the inversion amplifies by cond(R) (~1e5 here) -> normwise 1e-4 (the
        # north-star tolerance)
        for g, w in zip(inv, want_inv):
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-4 * np.abs(w).max())
            assert np.all(np.triu(g, 1) == 0)
    for a, b in zip(results[0][2], results[-1][2]):  # every rank holds the same L factors
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("shape,shard,lf,side", [("small", False, 1, True), ("c4", False, 1, True),
                                                 ("small", True, 1, True), ("c4", False, 16, True),
                                                 ("c4", False, 16, False)])
def test_two_ranks_match_single_device(hip_device, shape, shard, lf, side):
    results = _run(2, shape, shard, launch_first=lf, side=side)
    want_st, want_inv = _single_device(hip_device, shape)
    _check(results, want_st, want_inv, shard, side, expect_side=side and lf == 16)


def test_two_ranks_accumulate_without_reset(hip_device):
    """Two passes with no reset() in between (update, invert, update, invert), one
    launch per pass: pass 1's collective runs on the inversion's side stream, pass 2
    adds its all-reduced factors into that state on the caller's stream.  Equals one
    device accumulating both passes."""
    results = _run(2, "small", False, launch_first=16, accumulate=True)
    want_st, want_inv = _single_device(hip_device, "small", passes=2)
    _check(results, want_st, want_inv, False, expect_side=True)


@pytest.mark.parametrize("shard,lf", [(False, 1), (True, 1), (False, 16)])
def test_rccl_world1_collectives(hip_device, shard, lf):
    """The RCCL (nccl backend) all-reduce of the packed triangles and, sharded, the
    all-gather of the L factors, at world 1: results equal plain KFAC's.  With one
    launch per pass (lf 16) the all-reduce runs on the inversion's side stream."""
    results = _run(1, "small", shard, backend="nccl", launch_first=lf)
    want_st, want_inv = _single_device(hip_device, "small")
    _check(results, want_st, want_inv, shard, expect_side=lf == 16 and not shard)


@pytest.mark.parametrize("shape,shard", [("small", False), ("c4", False), ("small", True)])
def test_rccl_two_ranks_two_gpus(hip_device, shape, shard):
    """C4's path as the 8-GPU bench runs it: world 2 over RCCL, one rank per GPU
    (skipped on a one-GPU box; the driver's multi-GPU node runs it)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs (one RCCL rank per GPU)")
    results = _run(2, shape, shard, backend="nccl", launch_first=16)
    want_st, want_inv = _single_device(hip_device, shape)
    _check(results, want_st, want_inv, shard, expect_side=not shard)


def test_bench_two_ranks_parity_field(tmp_path):
    """`bench.py --gpus 2 --full` end to end on one device (--shared-device: gloo instead
    of RCCL, both ranks on GPU 0): the JSON line carries the post-timing verification
    pass's verdict (a --full leg), and it is true."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--shared-device",
                          "--full", "--steps", "2", "--warmup", "1", "--no-serial", "--images", "32768"],
                         capture_output=True, text=True, timeout=240, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and "shared device" in line["config"]["parallelism"]
    assert line["parity"] is True, line["parity_detail"]
    d = line["parity_detail"]
    assert d["records_checksum_match"] and d["identical_L_all_ranks"]
    assert d["max_rel_err_factors"] <= 1e-5 and d["max_rel_err_L"] <= 1e-4


@pytest.mark.parametrize("sizes", [(1, 10, 64, 65), (785, 128, 129, 10), (4097, 33)])
def test_tri_pack_unpack_roundtrip(hip_device, sizes):
    from bnn_kfac_amd import _native as N
    rng = np.random.default_rng(sum(sizes))
    mats = [torch.from_numpy(rng.standard_normal((n, n)).astype(np.float32)).to(hip_device)
            for n in sizes]
    jobs, total = N.tri_jobs(mats)
    packed = torch.full((total,), float("nan"), device=hip_device)
    N.tri_pack(jobs, packed)
    want = np.concatenate([m.cpu().numpy()[np.tril_indices(m.shape[0])] for m in mats])
    np.testing.assert_array_equal(packed.cpu().numpy(), want)
    for mode in (N.TRI_SYMMETRIC, N.TRI_LOWER):
        outs = [torch.full_like(m, float("nan")) for m in mats]
        N.tri_unpack(N.tri_jobs(outs)[0], packed, mode)
        for m, o in zip(mats, outs):
            low = np.tril(m.cpu().numpy())
            exp = low + np.tril(low, -1).T if mode == N.TRI_SYMMETRIC else low
            np.testing.assert_array_equal(o.cpu().numpy(), exp)
