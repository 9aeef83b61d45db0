"""The multi-GPU learner-update path on the GPU: agent-parallel LR-TS and learning-bidder
updates (sharding.lrts_update_agent_parallel / bidder_update_agent_parallel, what bench.py
runs at N > 1 over RCCL) with 2 ranks sharing cuda:0 over gloo (the box has one GPU; gloo
stages the device stores through host memory). Each rank simulates its shard of global
auction indices of the bench's mixed population (configs[4]: Oracle, LR-TS and
DoublyRobust bidders), collects its records, and the update routes them to their agent's
owner. Every rank must end with exactly the models of one process that simulated and
trained on all auctions (src/Agent.py:79-94, src/main.py:127-128)."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, B, out_path):
    import sys
    for p in (os.path.join(ROOT, "auction-gym_amd"), ROOT):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import bench
    from auctiongym_amd.sharding import (bidder_update_agent_parallel, lrts_update_agent_parallel,
                                         shard_range)
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    eng, what, _, ak, bk, st16, dims = bench.build_population("configs_4", 0)
    lo, hi = shard_range(B, rank, world)
    n = hi - lo
    inp = eng.alloc_inputs(n)
    eng.generate(0, lo, inp)
    eng.generate_noise(0, lo, inp)
    out = eng.alloc_outputs(n)
    eng.simulate(inp, out, eng.new_counters())
    lst = eng.new_lrts_samples(n)
    sst = eng.new_shading_samples(n * dims["P"], learning=True)
    eng.lrts_collect(inp, out, lst)
    eng.shading_collect(inp, out, sst, first_auction=lo)
    N = dims["N"]
    lep = lrts_update_agent_parallel(eng, lst, [a for a in range(N) if ak[a] == 1])
    ep, stat = bidder_update_agent_parallel(eng, sst, [a for a in range(N) if bk[a] >= 2])
    m, q, pm = eng.lrts_state()
    state, init = eng.dr_state()
    np.savez(out_path + f".{world}.{rank}.npz", m=m, q=q, pm=pm, state=state, init=init, lep=np.asarray(lep),
             ep=ep, stat=stat)
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_agent_parallel_updates_equal_single_process(gpu, tmp_path):
    B = 1 << 15
    out = str(tmp_path / "ap")
    mp.spawn(_worker, args=(1, 0, B, out), nprocs=1, join=True)
    mp.spawn(_worker, args=(2, _free_port(), B, out), nprocs=2, join=True)
    ref = np.load(out + ".1.0.npz")
    assert (ref["stat"] == 0).all() and ref["ep"].max() > 0 and ref["lep"].max() > 0
    for r in range(2):
        got = np.load(out + f".2.{r}.npz")
        for k in ("m", "q", "pm", "state", "init", "lep", "ep", "stat"):
            assert np.array_equal(got[k], ref[k]), (r, k)


def test_bench_multi_rank_rehearsal(gpu, tmp_path):
    """bench.py's N > 1 path end to end -- shards, the exact counter all-reduce, the
    agent-parallel learner updates of configs[1..4] -- with 2 ranks sharing the box's GPU over
    gloo (`--rehearse-on-one-gpu`; the driver's multi-GPU runs use RCCL on one GPU per rank).
    Every rank must finish and rank 0 print one JSON line for 2 GPUs."""
    import json
    import subprocess
    import sys
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", str(1 << 20), "--ts-batch", str(1 << 16),
           "--no-cpu-baseline", "--no-generate", "--populations", "configs_4", "--rehearse-on-one-gpu"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=280, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0
    assert d["configs_1"]["agent_update"]["epochs"] and d["configs_4"]["agent_update"]["bidder_epochs"]


def _rp_worker(rank, world, port, B, out_path):
    import sys
    for p in (os.path.join(ROOT, "auction-gym_amd"), ROOT):
        sys.path.insert(0, p)
    import torch
    import torch.distributed as dist

    import bench
    from auctiongym_amd.sharding import bidder_update_agent_parallel, bidder_update_record_parallel
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    # FP_DR_TS (configs[3]): 3 DoublyRobust learners -- the A < G case record-parallel is for
    eng, what, _, ak, bk, st16, dims, lo, inp, out, cnt = bench.population_first_iteration(
        "configs_3", 0, batch=B // world, world=world, rank=rank)
    sst = eng.new_shading_samples(B // world * dims["P"], learning=True)
    eng.shading_collect(inp, out, sst, first_auction=lo)
    learners = [a for a in range(dims["N"]) if bk[a] >= 2]
    fn = bidder_update_agent_parallel if world == 1 else bidder_update_record_parallel
    ep, stat = fn(eng, sst, learners)
    state, init = eng.dr_state()
    np.savez(out_path + f".{world}.{rank}.npz", state=state, init=init, ep=ep, stat=stat)
    eng.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_record_parallel_bidder_update_equals_single_process(gpu, tmp_path):
    """sharding.bidder_update_record_parallel with 2 ranks sharing cuda:0 over gloo: each rank
    simulates its shard of FP_DR_TS's auctions and keeps its own records; the fits run one
    launch per epoch with each epoch's exact partials all-reduced. Every rank ends with exactly
    the models, epochs and status of one process that simulated and trained on all auctions
    (the persistent trainer)."""
    B = 1 << 14
    out = str(tmp_path / "rp")
    mp.spawn(_rp_worker, args=(1, 0, B, out), nprocs=1, join=True)
    mp.spawn(_rp_worker, args=(2, _free_port(), B, out), nprocs=2, join=True)
    ref = np.load(out + ".1.0.npz")
    assert (ref["stat"] == 0).all() and ref["ep"][:, 2].max() > 0
    for r in range(2):
        got = np.load(out + f".2.{r}.npz")
        for k in ("state", "init", "ep", "stat"):
            assert np.array_equal(got[k], ref[k]), (r, k)
