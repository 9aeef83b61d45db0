#!/usr/bin/env python3
"""Times ag_simulate_slots_generated beside the paths it fuses, on one GPU (DESIGN.md section 4,
generate mode for multi-slot rounds).

Per configuration, every output array and the counters written:
  * fused       ag_simulate_slots_generated: nothing but the catalogue read from HBM;
  * hbm         ag_simulate_slots on HBM-resident inputs drawn once (unchanged code: the baseline);
  * three-call  ag_generate (+ ag_generate_noise) + ag_generate_slots + ag_simulate_slots.
Configurations: an OracleAllocator + TruthfulBidder population (N = 12, K = 12, E = 5, P = 8) at
max_slots 2 and 8, B = 2^--log2-auctions; and the shipped-shape mixed population (LR-TS sampling,
EmpiricalShaded, DoublyRobust uninitialised and fitted, a fitted PolicyLearning bidder; N = 10,
P = 3, max_slots = 3) -- the three variants at B = 2^--mixed-log2-auctions, where its Thompson
noise (720 B per auction) fits HBM, and the fused call alone at the largest B the 32-bit SoA
indexing admits, B * max(P, max_slots) < 2^31, halved until its outputs fit half the free memory.
The variants of a configuration alternate round by round in rotating order; a figure is the median
over the rounds of a device-event window of about --window-ms of calls, after a warm-up.
Prints one JSON line per variant. --lib: another build of the same ABI (A/B of a build knob).

    python tools/slots_generated_timing.py [--configs mixed] [--lib build/variants/libauctiongym_hip_X.so]
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

from auctiongym_amd import _lib  # noqa: E402
from auctiongym_amd.engine import AuctionEngine  # noqa: E402

K, E, OE, MECH = 12, 5, 4, 1


def nbytes(tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def catalogue(g, N):
    items = np.concatenate([g.normal(0, 1, (N, K, E)), -3.0 - g.random((N, K, 1))], axis=2)
    return items, g.lognormal(0.1, 0.2, (N, K))


def oracle_engine(S, lib, N=12, P=8):
    g = np.random.default_rng(0)
    eng = AuctionEngine(N, P, K, E, OE, MECH, 1.0, lib_path=lib, max_slots=S)
    eng.load_catalog(*catalogue(g, N))
    return eng


def mixed_engine(S, lib, N=10, P=3):
    g = np.random.default_rng(1)
    eng = AuctionEngine(N, P, K, E, OE, MECH, 1.0, lib_path=lib, max_slots=S)
    ak = np.array([i % 2 for i in range(N)], np.int32)
    bk = np.array([0, 1, 4, 4, 2, 3, 0, 1, 4, 0], np.int32)
    init = np.array([0, 0, 0, 1, 1, 1, 0, 0, 1, 0], np.int32)
    eng.set_agent_params(ak, bk, 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N))
    eng.load_catalog(*catalogue(g, N))
    eng.load_lrts(g.normal(0, 1, (N, K, OE + 1)).astype(np.float32),
                  (1.0 + 3.0 * g.random((N, K, OE + 1))).astype(np.float32), thompson_sampling=True)
    eng.set_dr_state(g.normal(0, 0.7, (N, 16)).astype(np.float32), init)
    eng.set_bidder_modes(np.full(N, _lib.VL_POLICY, np.int32))
    return eng


def draw(eng, seed, inp):
    eng.generate(seed, 0, inp)
    if any(k in inp for k in ("gamma_raw", "ts_noise", "policy_eps")):
        eng.generate_noise(seed, 0, inp)
    eng.generate_slots(seed, 0, inp)


def window(f, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        f()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def run(config, B, variants, a):
    for _, f, _ in variants:  # warm-up: code objects loaded, grids sized
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    reps = [max(2, int(a.window_ms / window(f, 2))) for _, f, _ in variants]
    times = [[] for _ in variants]
    for r in range(a.rounds):  # the order rotates: no variant always follows the same neighbour
        for j in range(len(variants)):
            i = (j + r) % len(variants)
            times[i].append(window(variants[i][1], reps[i]))
    for (name, _, nb), t, r in zip(variants, times, reps):
        ms = statistics.median(t)
        print(json.dumps({"config": config, "variant": name, "auctions": B, "ms_per_call": round(ms, 4),
                          "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                          "Mauctions_per_s": round(B / ms / 1e3, 1), "hbm_bytes_per_call": nb,
                          "GB_per_s": round(nb / ms / 1e6, 1), "calls_timed": r * a.rounds,
                          "device": torch.cuda.get_device_name(0)}), flush=True)


def three_variants(eng, B):
    inp = eng.alloc_inputs(B)
    draw(eng, 1, inp)
    out, cnt = eng.alloc_slot_outputs(B), eng.new_counters()
    ob = nbytes(out.values())
    # u_slots rows are read for filled slots only: min(n, P - 1) per auction
    read_u = int(torch.clamp(inp["num_slots"], max=eng.P - 1).sum().item()) * 8
    ib = nbytes(v for k, v in inp.items() if k not in ("u", "u_slots")) + read_u
    gen_b = nbytes(inp.values())  # the three-call path writes every input, then reads what hbm reads

    def three():
        draw(eng, 1, inp)
        eng.simulate_slots(inp, inp["num_slots"], inp["u_slots"], out, cnt)

    return [("fused", lambda: eng.simulate_slots_generated(1, 0, out, cnt), ob),
            ("hbm", lambda: eng.simulate_slots(inp, inp["num_slots"], inp["u_slots"], out, cnt), ib + ob),
            ("three-call", three, gen_b + ib + ob)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-auctions", type=int, default=24)
    ap.add_argument("--mixed-log2-auctions", type=int, default=22)
    ap.add_argument("--window-ms", type=float, default=250.0, help="device time per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds (the median is reported)")
    ap.add_argument("--lib", default=None, help="another build of the same ABI")
    ap.add_argument("--configs", default="oracle,mixed,largest", help="which of oracle, mixed, largest to run")
    a = ap.parse_args()
    lib = os.path.abspath(a.lib) if a.lib else None
    configs = a.configs.split(",")
    for S in (2, 8) if "oracle" in configs else ():
        eng = oracle_engine(S, lib)
        B = 1 << a.log2_auctions
        run(f"oracle P=8 max_slots={S}", B, three_variants(eng, B), a)
        eng.close()
        torch.cuda.empty_cache()
    eng = mixed_engine(3, lib)
    if "mixed" in configs:
        B = 1 << a.mixed_log2_auctions
        run("mixed P=3 max_slots=3", B, three_variants(eng, B), a)
        torch.cuda.empty_cache()
    if "largest" in configs:
        B = ((2 ** 31 - 1) // max(eng.P, eng.max_slots)) & ~255
        per = nbytes(eng.alloc_slot_outputs(256).values()) // 256
        while B * per > torch.cuda.mem_get_info()[0] // 2:
            B //= 2
        out, cnt = eng.alloc_slot_outputs(B), eng.new_counters()
        run("mixed P=3 max_slots=3, largest B", B,
            [("fused", lambda: eng.simulate_slots_generated(1, 0, out, cnt), nbytes(out.values()))], a)
    eng.close()


if __name__ == "__main__":
    main()
