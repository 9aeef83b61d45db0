#!/usr/bin/env python3 -B
"""Golden vectors of multi-slot rounds (TEST INFRASTRUCTURE; runs only in the dev container).

The reference's Auction and both allocation mechanisms are written for num_slots slots; only its
main.py hard-codes max_slots = 1. This script builds the reference's auction as main.py does, with
max_slots passed in, and records per round what its hot path computes: the slot count, the doubles
rng.binomial consumes, the replay inputs, every participant's log fields, allocate's three arrays,
and the per-agent utilities, regrets and the revenue. Shims and config helpers are make_golden.py's,
imported; nothing from the reference is copied: the files written are data.

Draw order, asserted on every round: a clone of the reference's Generator (and, where the
population draws from torch, a saved copy of torch's generator state) is advanced as
    n = integers(1, max_slots + 1); normal(0, var, E); choice(N, P, replace=False);
    per participant, in slot order: the LR-TS Thompson draw torch.normal(0, 1/sqrt(q)), then an
    EmpiricalShadedBidder's normal(prev_gamma, gamma_sigma);
    min(n, P) x random()  -- one per element of binomial(1, CTRs[winners])
and must end in the reference's state(s).

A fixture is refused (pick another seed) when a round has an exact tie among its top F + 1 bids, a
winner whose true CTR is 0, or a (p, u) at which numpy's exp(log(q)) threshold and the kernels'
1 - p / p threshold give different clicks.

Usage:  python3 -B tests/golden/make_golden_slots.py
"""
import json
import math
import os

import numpy as np

import make_golden as MG

OUT = MG.OUT
ROUNDS = 1024

ORACLE_SHAPES = ((4, 3), (2, 3), (3, 8), (1, 2))  # (P, max_slots), N = 6, K = 12, seed 3


def kernel_bernoulli(p, u):
    """The kernels' click rule (csrc/ag_sim.h bernoulli)."""
    if p == 0.0:
        return 0
    if p <= 0.5:
        return int(u > 1.0 - p)
    return 0 if u > p else 1


def numpy_bernoulli(p, u):
    """numpy's binomial(1, p) from its double u (inversion, n = 1)."""
    if p == 0.0:
        return 0
    if p <= 0.5:
        return int(u > math.exp(math.log(1.0 - p)))
    q = 1.0 - p
    return 1 - int(u > math.exp(math.log(1.0 - q)))


def capture_slots(cfg, max_slots, rounds=ROUNDS, torch_seed=0):
    import main as M
    import torch
    path = MG.write_cfg(cfg)
    (rng, config, agent_configs, agents2items, agents2item_values, _, _, E, var, OE) = M.parse_config(path)
    os.unlink(path)
    torch.manual_seed(torch_seed)
    agents = M.instantiate_agents(rng, agent_configs, agents2item_values, agents2items)
    auction, _, _, _ = M.instantiate_auction(rng, config, agents2items, agents2item_values, agents, max_slots,
                                             E, var, OE)
    N, P, S = len(agents), config["num_participants_per_round"], max_slots
    names = [a.name for a in agents]
    K = len(agents2item_values[names[0]])
    items = np.stack([agents2items[n] for n in names])
    values = np.stack([agents2item_values[n] for n in names])
    is_ts = [type(a.allocator).__name__ == "PyTorchLogisticRegressionAllocator" for a in agents]
    shading = [hasattr(a.bidder, "prev_gamma") for a in agents]
    Do = ts_m = ts_q = None
    if any(is_ts):
        Do = agents[is_ts.index(True)].allocator.response_model.m.shape[1]
        ts_m = np.stack([a.allocator.response_model.m.detach().numpy() if is_ts[i] else np.zeros((K, Do), np.float32)
                         for i, a in enumerate(agents)])
        ts_q = np.stack([a.allocator.response_model.q.numpy() if is_ts[i] else np.ones((K, Do), np.float32)
                         for i, a in enumerate(agents)])

    clone = np.random.Generator(np.random.PCG64())
    clone.bit_generator.state = rng.bit_generator.state
    alloc_log = []
    orig = auction.allocation.allocate

    def wrapped(bids, num_slots):
        w, p, s = orig(bids, num_slots)
        alloc_log.append((int(num_slots), np.array(bids, np.float64), np.array(w), np.array(p), np.array(s)))
        return w, p, s

    auction.allocation.allocate = wrapped
    noise_log = []
    orig_normal = torch.normal

    def rec_normal(*a, **k):
        t = orig_normal(*a, **k)
        noise_log.append(t.detach().numpy().copy())
        return t

    torch.normal = rec_normal
    R, U = rounds, min(S, P)
    ctx = np.zeros((R, E))
    part = np.zeros((R, P), np.int32)
    num_slots = np.zeros(R, np.int32)
    u_slots = np.full((R, U), np.nan)
    gamma_raw = np.full((R, P), np.nan)
    ts_noise = np.zeros((R, P, K, Do), np.float32) if Do else None
    rec = {k: np.zeros((R, P)) for k in ("bid", "est_ctr", "true_ctr", "best_ev", "value", "price", "second_price",
                                         "gamma")}
    item = np.zeros((R, P), np.int32)
    won = np.zeros((R, P), np.int8)
    outcome = np.zeros((R, P), np.int8)
    aw = np.full((R, S), -1, np.int32)
    ap = np.full((R, S), np.nan)
    asec = np.full((R, S), np.nan)
    try:
        for r in range(R):
            ts0 = torch.get_rng_state()
            n = int(clone.integers(1, S + 1))
            c = clone.normal(0, var, size=E)
            pa = clone.choice(N, P, replace=False)
            for s_, a_ in enumerate(pa):
                if shading[a_]:
                    b = agents[a_].bidder
                    gamma_raw[r, s_] = clone.normal(b.prev_gamma, b.gamma_sigma)
            us = [clone.random() for _ in range(min(n, P))]
            n0 = len(noise_log)
            auction.simulate_opportunity()
            assert clone.bit_generator.state == rng.bit_generator.state, f"draw order diverged at round {r}"
            nts = [s_ for s_, a_ in enumerate(pa) if is_ts[a_] and agents[a_].allocator.thompson_sampling]
            assert len(noise_log) - n0 == len(nts)
            if nts:  # torch's generator: the same draws again from the saved state end in the same state
                ts1 = torch.get_rng_state()
                torch.set_rng_state(ts0)
                for j, s_ in enumerate(nts):
                    q = agents[pa[s_]].allocator.response_model.q
                    z = orig_normal(mean=0.0, std=1.0 / torch.sqrt(q)).numpy()
                    assert np.array_equal(z, noise_log[n0 + j]), f"Thompson draw order diverged at round {r}"
                    ts_noise[r, s_] = z
                assert torch.equal(torch.get_rng_state(), ts1), f"torch draw order diverged at round {r}"
            ctx[r], part[r], num_slots[r] = c, pa, n
            u_slots[r, :len(us)] = us
            for s, a in enumerate(pa):
                lg = agents[a].logs[-1]
                rec["bid"][r, s], rec["est_ctr"][r, s], rec["true_ctr"][r, s] = lg.bid, lg.estimated_CTR, lg.true_CTR
                rec["best_ev"][r, s], rec["value"][r, s] = lg.best_expected_value, lg.value
                rec["price"][r, s], rec["second_price"][r, s] = lg.price, lg.second_price
                rec["gamma"][r, s] = float(agents[a].bidder.gammas[-1]) if shading[a] else np.nan
                item[r, s], won[r, s], outcome[r, s] = lg.item, bool(lg.won), bool(lg.outcome)
            ns, bids, w, p, s2 = alloc_log[-1]
            assert ns == n and np.array_equal(bids, rec["bid"][r])
            aw[r, :len(w)], ap[r, :len(p)], asec[r, :len(s2)] = w, p, s2
            # the fixture's conditions
            F = min(n, P - 1)
            top = np.sort(bids)[::-1][:F + 1]
            assert len(set(top.tolist())) == len(top), f"round {r}: exact tie among the top F + 1 bids"
            for k, wk in enumerate(w):
                pk = float(rec["true_ctr"][r, wk])
                assert pk != 0.0, f"round {r}: a winner with true CTR 0"
                assert kernel_bernoulli(pk, us[k]) == numpy_bernoulli(pk, us[k]), \
                    f"round {r}: numpy's and the kernels' click thresholds differ at (p, u) = ({pk!r}, {us[k]!r})"
                if k < F:
                    assert int(outcome[r, wk]) == numpy_bernoulli(pk, us[k])
    finally:
        torch.normal = orig_normal
    st = rng.bit_generator.state
    agg = {"net_utility": [a.net_utility for a in agents], "gross_utility": [a.gross_utility for a in agents],
           "revenue": auction.revenue,
           "allocation_regret": [float(a.get_allocation_regret()) for a in agents],
           "estimation_regret": [float(a.get_estimation_regret()) for a in agents],
           "overbid_regret": [float(a.get_overbid_regret()) for a in agents],
           "underbid_regret": [float(a.get_underbid_regret()) for a in agents],
           "n_logs": [len(a.logs) for a in agents],
           "rng_state_after": {"state": str(st["state"]["state"]), "inc": str(st["state"]["inc"]),
                               "has_uint32": int(st["has_uint32"]), "uinteger": int(st["uinteger"])}}
    arrays = dict(items=items, values=values, ctx=ctx, part=part, num_slots=num_slots, u_slots=u_slots,
                  gamma_raw=gamma_raw, item=item, won=won, outcome=outcome, alloc_winner=aw, alloc_price=ap,
                  alloc_second=asec, **{"slot_" + k: v for k, v in rec.items()})
    if Do:
        arrays.update(ts_noise=ts_noise, ts_m=ts_m, ts_q=ts_q)
    meta = dict(N=N, P=P, K=K, E=E, OE=OE, var=var, rounds=R, max_slots=S, allocation=config["allocation"],
                seed=config["random_seed"], torch_seed=torch_seed,
                allocators=[type(a.allocator).__name__ for a in agents], bidders=[type(a.bidder).__name__ for a in agents],
                bidder_kwargs=[c["bidder"]["kwargs"] for c in agent_configs], ts_dim=Do, num_items=[K] * N, config=cfg)
    return arrays, agg, meta


def save(name, arrays, agg, meta):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    if os.path.getsize(path) > 1 << 20 and "ts_noise" in arrays:  # as make_golden.save_capture
        np.savez_compressed(path, **{k: v for k, v in arrays.items() if k != "ts_noise"})
        np.savez_compressed(os.path.join(OUT, name + ".ts_noise.npz"), ts_noise=arrays["ts_noise"])
    for f in (name + ".npz", name + ".ts_noise.npz"):
        p = os.path.join(OUT, f)
        assert not os.path.exists(p) or os.path.getsize(p) <= 1 << 20, f"{f} is larger than 1 MiB"
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump({"meta": meta, "aggregates": agg}, f, indent=1)
    print("wrote", name, os.path.getsize(path), "bytes")


def main():
    MG.install_shims()
    for P, S in ORACLE_SHAPES:
        for mech, tag in (("FirstPrice", "fp"), ("SecondPrice", "sp")):
            a, g, m = capture_slots(MG.oracle_truthful_cfg(6, 12, P, mech, seed=3), S)
            save(f"slots_{tag}_oracle_p{P}_s{S}", a, g, m)
    # EmpiricalShadedBidder (numpy-only bidder draws), P = 3, max_slots 3
    cfg = MG.oracle_truthful_cfg(6, 12, 3, "FirstPrice", seed=3)
    cfg["agents"][0]["bidder"] = {"type": "EmpiricalShadedBidder", "kwargs": {"gamma_sigma": 0.05, "init_gamma": 0.9}}
    a, g, m = capture_slots(cfg, 3)
    save("slots_fp_empirical_p3_s3", a, g, m)
    # SP_Truthful_TS (torch Thompson draws) at P = 3, max_slots 3
    cfg = MG.load_cfg("SP_Truthful_TS.json", num_participants_per_round=3, random_seed=3)
    a, g, m = capture_slots(cfg, 3)
    save("slots_sp_ts_p3_s3", a, g, m)


if __name__ == "__main__":
    main()
