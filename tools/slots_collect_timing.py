#!/usr/bin/env python3
"""Times the record collectors of multi-slot rounds on one GPU.

Two populations of N = 6 agents, K = 12, E = 5, OE = 4, P = 4 at B = 2^22 synthetic auctions
(ag_generate, ag_generate_noise), simulated once per context:
  * sp_ts         LR-TS allocators (MAP item choice: no Thompson noise to hold) with TruthfulBidders
                  over SecondPrice -> ag_lrts_collect_slots;
  * fp_empirical  OracleAllocators with EmpiricalShadedBidders over FirstPrice ->
                  ag_shading_collect_slots into an (agent, gamma, utility) store;
on contexts of max_slots 1, 3 and 8 (slot counts uniform in 1..max_slots). At max_slots = 1 the
one-slot collectors (ag_lrts_collect, ag_shading_collect) run on ag_simulate's outputs of the same
inputs: the yardstick. Every timed call resets the store's count first (one 8-byte memset, in every
variant), so no call overflows its store.
The variants alternate round by round, in rotating order; every figure is the median over the rounds
of a device-event window of about --window-ms of calls, after a warm-up. Prints one JSON line per
variant: ms per call, the records appended, the bytes a call moves per auction (arrays read once,
records written) and the rate they give.

    python tools/slots_collect_timing.py
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

N, K, E, OE, P = 6, 12, 5, 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-auctions", type=int, default=22)
    ap.add_argument("--window-ms", type=float, default=100.0, help="device time per timed window")
    ap.add_argument("--rounds", type=int, default=7, help="alternating rounds (the median is reported)")
    a = ap.parse_args()
    B = 1 << a.log2_auctions
    g = np.random.default_rng(0)
    items = np.concatenate([g.normal(0, 1, (N, K, E)), -3.0 - g.random((N, K, 1))], axis=2)
    values = g.lognormal(0.1, 0.2, (N, K))
    m = g.normal(0, 1, (N, K, OE + 1)).astype(np.float32)
    variants = []

    def engine(pop, S):
        ts = pop == "sp_ts"
        eng = AuctionEngine(N, P, K, E, OE, 1 if ts else 0, 1.0, max_slots=S)
        eng.set_agent_params(np.full(N, int(ts), np.int32), np.full(N, int(not ts), np.int32), np.full(N, 0.9),
                             np.full(N, 0.05))
        eng.load_catalog(items, values)
        if ts:
            eng.load_lrts(m, np.ones_like(m), thompson_sampling=False)
        return eng

    def add(name, call, store, records, nbytes):
        def f():
            store["count"].zero_()
            call()
        variants.append((name, f, records, nbytes))

    for pop in ("sp_ts", "fp_empirical"):
        ts = pop == "sp_ts"
        inp = None
        for S in (1, 3, 8):
            eng = engine(pop, S)
            if inp is None:  # the same inputs for every context of the population
                inp = eng.alloc_inputs(B)
                eng.generate(1, 0, inp)
                if "gamma_raw" in inp:
                    eng.generate_noise(1, 0, inp)
            ns = torch.from_numpy(g.integers(1, S + 1, B).astype(np.int32)).to(eng.device)
            us = inp["u"].view(1, B) if S == 1 else torch.rand((min(S, P), B), dtype=torch.float64, device=eng.device)
            out = eng.alloc_slot_outputs(B)
            eng.simulate_slots(inp, ns, us.contiguous(), out)
            filled = int(out["num_filled"].sum().item())
            if ts:
                st = eng.new_lrts_samples(B * min(S, P - 1))
                eng.lrts_collect_slots(inp, out, st)
                rec = int(st["count"].item())
                # num_filled; per filled slot winner, outcome, part, item; the OE context doubles of an
                # auction with a record (every one here); per record key + OE + 1 floats
                nb = B * 4 + filled * (4 + 1 + 4 + 4) + B * OE * 8 + rec * (4 + (OE + 1) * 4)
                add(f"{pop}: ag_lrts_collect_slots, max_slots={S}",
                    lambda eng=eng, out=out, st=st: eng.lrts_collect_slots(inp, out, st), st, rec, nb)
            else:
                st = eng.new_shading_samples(B * P)
                eng.shading_collect_slots(inp, out, st)
                rec = int(st["count"].item())
                # part; log_price; per record won_slot, item, gamma (+ the click of a winner); per
                # record agent, gamma, utility
                nb = B * P * 4 + B * 8 + rec * (1 + 4 + 8) + filled + rec * (4 + 8 + 8)
                add(f"{pop}: ag_shading_collect_slots, max_slots={S}",
                    lambda eng=eng, out=out, st=st: eng.shading_collect_slots(inp, out, st), st, rec, nb)
            if S > 1:
                continue
            out1 = eng.alloc_outputs(B)
            eng.simulate(inp, out1)
            if ts:
                s1 = eng.new_lrts_samples(B)
                eng.lrts_collect(inp, out1, s1)
                r1 = int(s1["count"].item())
                nb = B * (4 + 1 + 4 + 4) + B * OE * 8 + r1 * (4 + (OE + 1) * 4)
                add(f"{pop}: ag_lrts_collect (one slot)",
                    lambda eng=eng, out1=out1, s1=s1: eng.lrts_collect(inp, out1, s1), s1, r1, nb)
            else:
                s1 = eng.new_shading_samples(B * P)
                eng.shading_collect(inp, out1, s1)
                r1 = int(s1["count"].item())
                nb = B * P * 4 + B * (4 + 1 + 8) + r1 * (4 + 8) + r1 * (4 + 8 + 8)
                add(f"{pop}: ag_shading_collect (one slot)",
                    lambda eng=eng, out1=out1, s1=s1: eng.shading_collect(inp, out1, s1, 0), s1, r1, nb)
            assert r1 == rec, (r1, rec)
    for _, f, _, _ in variants:  # warm-up
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

    reps = [max(5, int(a.window_ms / window(f, 5))) for _, f, _, _ in variants]
    times = [[] for _ in variants]
    for r in range(a.rounds):  # the order rotates: no variant always follows the same neighbour
        for j in range(len(variants)):
            i = (j + r) % len(variants)
            times[i].append(window(variants[i][1], reps[i]))
    for (name, _, rec, nb), t, r in zip(variants, times, reps):
        ms = statistics.median(t)
        print(json.dumps({"variant": name, "auctions": B, "records": rec, "ms_per_call": round(ms, 4),
                          "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                          "bytes_per_auction": round(nb / B, 1), "GB_per_s": round(nb / ms / 1e6, 1),
                          "calls_timed": r * a.rounds, "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
