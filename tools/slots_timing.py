#!/usr/bin/env python3
"""Times ag_simulate_slots beside ag_simulate on one GPU (multi-slot rounds).

An OracleAllocator + TruthfulBidder population at N = 6, K = 12, E = 5, P = 4, B = 2^22 synthetic
auctions (ag_generate), every output array and the counters written:
  * ag_simulate_slots on contexts of max_slots 1, 3 and 8 (slot counts uniform in 1..max_slots);
  * ag_simulate on the same inputs, this build -- and, with --parent-lib, another build of the same
    ABI (the parent commit's library), to show that the one-slot path did not move.
The variants alternate round by round, in rotating order; every figure is the median over the rounds of a
device-event window of about --window-ms of calls (7 x 250 ms of work per figure at the defaults),
after a warm-up.
Prints one JSON line per variant: ms per call, the bytes a call moves, and the rate they give.

    python tools/slots_timing.py [--parent-lib build/variants/libauctiongym_hip_parent.so]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "auction-gym_amd"))

from auctiongym_amd.engine import AuctionEngine  # noqa: E402

N, K, E, OE, P, MECH = 6, 12, 5, 4, 4, 1


def nbytes(tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-auctions", type=int, default=22)
    ap.add_argument("--window-ms", type=float, default=250.0, help="device time per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (the median is reported)")
    ap.add_argument("--parent-lib", default=None, help="another build of the same ABI: its ag_simulate is timed too")
    a = ap.parse_args()
    B = 1 << a.log2_auctions
    g = np.random.default_rng(0)
    items = np.concatenate([g.normal(0, 1, (N, K, E)), -3.0 - g.random((N, K, 1))], axis=2)
    values = g.lognormal(0.1, 0.2, (N, K))
    variants = []

    def engine(max_slots=1, lib=None):
        eng = AuctionEngine(N, P, K, E, OE, MECH, 1.0, lib_path=lib, **({} if lib else {"max_slots": max_slots}))
        eng.load_catalog(items, values)
        return eng

    base = engine()
    inp = base.alloc_inputs(B)
    base.generate(1, 0, inp)
    in_bytes = nbytes([inp["ctx"], inp["part"]])

    out1, cnt1 = base.alloc_outputs(B), base.new_counters()  # shared by the one-slot variants: same addresses

    def one_slot(name, lib=None):
        # the default dispatch (k_oracle for this population) and the general kernel k_simulate,
        # which the multi-slot builds extend
        for generic, tag in ((False, ""), (True, ", AG_SIM_KERNEL_GENERIC")):
            eng = engine(lib=lib)
            eng.set_simulate_kernel(generic)
            out, cnt = out1, cnt1
            variants.append((name + tag, lambda eng=eng, out=out, cnt=cnt: eng.simulate(inp, out, cnt),
                             in_bytes + nbytes([inp["u"]]) + nbytes(out.values())))

    one_slot("ag_simulate")
    if a.parent_lib:
        one_slot("ag_simulate, parent build", os.path.abspath(a.parent_lib))
    for S in (1, 3, 8):
        eng = engine(S)
        ns = torch.from_numpy(g.integers(1, S + 1, B).astype(np.int32)).to(eng.device)
        us = torch.rand((min(S, P), B), dtype=torch.float64, device=eng.device)
        out, cnt = eng.alloc_slot_outputs(B), eng.new_counters()
        # u_slots rows are read for filled slots only: min(n, P - 1) per auction
        read_u = int(torch.minimum(ns, torch.tensor(P - 1, device=eng.device)).sum().item()) * 8
        variants.append((f"ag_simulate_slots, max_slots={S}",
                         lambda eng=eng, ns=ns, us=us, out=out, cnt=cnt: eng.simulate_slots(inp, ns, us, out, cnt),
                         in_bytes + nbytes([ns]) + read_u + nbytes(out.values())))
    for _, f, _ in variants:  # warm-up: code objects loaded, grids sized
        for _ in range(3):
            f()
    torch.cuda.synchronize()

    def window(f, reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            f()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / reps

    reps = [max(5, int(a.window_ms / window(f, 5))) for _, f, _ in variants]
    times = [[] for _ in variants]
    for r in range(a.rounds):  # the order rotates: no variant always follows the same neighbour
        for j in range(len(variants)):
            i = (j + r) % len(variants)
            times[i].append(window(variants[i][1], reps[i]))
    for (name, _, nb), t, r in zip(variants, times, reps):
        ms = statistics.median(t)
        print(json.dumps({"variant": name, "auctions": B, "ms_per_call": round(ms, 4), "min_ms": round(min(t), 4),
                          "max_ms": round(max(t), 4), "bytes_per_call": nb, "GB_per_s": round(nb / ms / 1e6, 1),
                          "calls_timed": r * a.rounds, "work_s": round(ms * r * a.rounds / 1e3, 2),
                          "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
