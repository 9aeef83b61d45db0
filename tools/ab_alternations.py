#!/usr/bin/env python3
"""A/B of library builds of the same ABI on the bench headline (SP_Oracle, HEADLINE_FIELDS),
as alternations: each alternation times every build in turn, STEPS calls each (device events
around each ag_simulate call, as bench.py's kernel_ms), and gives one median per build.

    python tools/ab_alternations.py parent=path/to/lib.so [name=path ...]
    (an arm named name@N runs with N resident workgroups per CU)
    AB_LOG2B (27), AB_ALTERNATIONS (7), AB_STEPS (20)

Prints one raw line per (alternation, build), then per build the median of its medians and
their spread (max - min), and whether every build's outputs and counters equal the first's.
The product build (auctiongym_amd/libauctiongym_hip.so) is always the arm "new".
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "auction-gym_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from auctiongym_amd import _lib  # noqa: E402
from auctiongym_amd.engine import HEADLINE_FIELDS, AuctionEngine  # noqa: E402


def main():
    paths = dict(a.split("=", 1) for a in sys.argv[1:])
    paths["new"] = _lib.LIB_PATH
    B = 1 << int(os.environ.get("AB_LOG2B", "27"))
    alternations = int(os.environ.get("AB_ALTERNATIONS", "7"))
    steps = int(os.environ.get("AB_STEPS", "20"))
    items, values = bench.catalogue()
    engs = {}
    for n, p in paths.items():
        e = AuctionEngine(6, 2, 12, 5, 4, _lib.SECOND_PRICE, 1.0, device=0, lib_path=os.path.abspath(p))
        e.load_catalog(items, values)
        if "@" in n:  # name@N: N resident workgroups per CU (AG_OPT_SIM_BLOCKS_PER_CU)
            e.set_blocks_per_cu(int(n.split("@")[1]))
        engs[n] = e
    first = next(iter(engs.values()))
    inp = first.alloc_inputs(B)
    first.generate(0, 0, inp)
    ref, cref = first.alloc_outputs(B, HEADLINE_FIELDS), first.new_counters()
    first.simulate(inp, ref, cref)
    out, cnt = first.alloc_outputs(B, HEADLINE_FIELDS), first.new_counters()
    for n, e in engs.items():
        for t in out.values():
            t.view(torch.uint8).fill_(0xA5)
        cnt.zero_()
        e.simulate(inp, out, cnt)
        torch.cuda.synchronize()
        same = all(torch.equal(out[k].view(torch.uint8), ref[k].view(torch.uint8)) for k in HEADLINE_FIELDS)
        print(f"{n}: outputs and counters identical to {next(iter(engs))}: {same and torch.equal(cnt, cref)}", flush=True)
    st = torch.cuda.current_stream()
    for _ in range(60):  # bench.py's default warm-up: past the clock ramp of a fresh process
        first.simulate(inp, out, cnt)
    torch.cuda.synchronize()
    med = {n: [] for n in engs}
    for alt in range(alternations):
        for n, e in engs.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for a, b in ev:
                cnt.zero_()
                a.record(st)
                e.simulate(inp, out, cnt)
                b.record(st)
            torch.cuda.synchronize()
            t = [a.elapsed_time(b) for a, b in ev]
            med[n].append(float(np.median(t)))
            print(f"alt {alt} {n:10s} median {med[n][-1]:.4f} ms  min {min(t):.4f}  max {max(t):.4f}  ({steps} steps, B = {B})",
                  flush=True)
    for n, m in med.items():
        print(f"{n:10s} median of medians {float(np.median(m)):.4f} ms  spread (max - min) {max(m) - min(m):.4f} ms")


if __name__ == "__main__":
    main()
