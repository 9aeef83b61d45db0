#!/usr/bin/env python3 -B
"""Golden vectors of the driver loop on multi-slot rounds (TEST INFRASTRUCTURE; runs only in the
dev container).

The reference's driver loop (src/main.py:113-155: the rounds, then per agent update, clear_utility,
clear_logs) with max_slots = 3 passed to its Auction, as make_golden_slots.py builds it, for 3
iterations of 1000 rounds, on two populations of learners:

  slots_update_fp_empirical   six EmpiricalShadedBidders over FirstPrice, P = 3
  slots_update_sp_ts          SP_Truthful_TS (LR-TS allocators, TruthfulBidders), P = 3

Recorded per iteration: every agent's prev_gamma before / after its update, the utilities, the four
regrets and the revenue, the numpy Generator's state after the rounds and, for the LR-TS
allocators, the inputs of every PyTorchLogisticRegressionAllocator.update (the won contexts as
float32, items, outcomes). Shims and config helpers are make_golden.py's, the click rules
make_golden_slots.py's, imported; nothing from the reference is copied: the files written are data.

A capture is refused (pick another seed) on what make_golden_slots.py refuses: a round with an
exact tie among its top F + 1 bids, a winner whose true CTR is 0, or a (p, u) at which numpy's
exp(log(q)) threshold and the kernels' 1 - p / p threshold give different clicks. The doubles
rng.binomial consumes come from a clone of the reference's Generator advanced in the draw order
make_golden_slots.py states, which must end every round in the reference's state.

Usage:  python3 -B tests/golden/make_golden_slots_update.py
"""
import json
import os

import numpy as np

import make_golden as MG
from make_golden_slots import kernel_bernoulli, numpy_bernoulli

OUT = MG.OUT
MAX_SLOTS, ITERS, ROUNDS = 3, 3, 1000


def capture_update(cfg, name, torch_seed=0):
    import main as M
    import torch
    cfg = dict(cfg, num_runs=1, num_iter=ITERS, rounds_per_iter=ROUNDS)
    path = MG.write_cfg(cfg)
    (rng, config, agent_configs, a2i, a2v, _, _, E, var, OE) = M.parse_config(path)
    os.unlink(path)
    torch.manual_seed(torch_seed)
    agents = M.instantiate_agents(rng, agent_configs, a2v, a2i)
    auction, _, _, _ = M.instantiate_auction(rng, config, a2i, a2v, agents, MAX_SLOTS, E, var, OE)
    N, P, S = len(agents), config["num_participants_per_round"], MAX_SLOTS
    shading = [hasattr(a.bidder, "prev_gamma") for a in agents]
    is_ts = [type(a.allocator).__name__ == "PyTorchLogisticRegressionAllocator" for a in agents]

    clone = np.random.Generator(np.random.PCG64())
    clone.bit_generator.state = rng.bit_generator.state
    last = {}
    orig = auction.allocation.allocate

    def wrapped(bids, num_slots):
        w, p, s = orig(bids, num_slots)
        last["alloc"] = (int(num_slots), np.array(bids, np.float64), np.array(w))
        return w, p, s

    auction.allocation.allocate = wrapped
    out = {}
    two_learners = overwritten = n_ge_p = 0
    for it in range(ITERS):
        for r in range(ROUNDS):
            n = int(clone.integers(1, S + 1))
            clone.normal(0, var, size=E)
            pa = clone.choice(N, P, replace=False)
            for a_ in pa:
                if shading[a_]:
                    clone.normal(agents[a_].bidder.prev_gamma, agents[a_].bidder.gamma_sigma)
            us = [clone.random() for _ in range(min(n, P))]
            auction.simulate_opportunity()
            assert clone.bit_generator.state == rng.bit_generator.state, f"draw order diverged at round {it}:{r}"
            ns, bids, w = last["alloc"]
            assert ns == n
            F = min(n, P - 1)
            top = np.sort(bids)[::-1][:F + 1]
            assert len(set(top.tolist())) == len(top), f"round {it}:{r}: exact tie among the top F + 1 bids"
            logs = [agents[a_].logs[-1] for a_ in pa]
            for k, wk in enumerate(w):
                pk = float(logs[wk].true_CTR)
                assert pk != 0.0, f"round {it}:{r}: a winner with true CTR 0"
                assert kernel_bernoulli(pk, us[k]) == numpy_bernoulli(pk, us[k]), \
                    f"round {it}:{r}: numpy's and the kernels' click thresholds differ at (p, u) = ({pk!r}, {us[k]!r})"
            won = [bool(lg.won) for lg in logs]
            assert sum(won) == F
            two_learners += sum(won) >= 2
            n_ge_p += n >= P
            own = np.sort(bids)[::-1] if config["allocation"] == "FirstPrice" else np.sort(bids)[::-1][1:]
            overwritten += sum(1 for k in range(F) if logs[w[k]].price != own[k])
        st = rng.bit_generator.state
        out[f"it{it}_np_state"] = np.array(json.dumps(
            {"state": str(st["state"]["state"]), "inc": str(st["state"]["inc"]), "has_uint32": int(st["has_uint32"]),
             "uinteger": int(st["uinteger"])}))
        out[f"it{it}_revenue"] = np.array(auction.revenue)
        out[f"it{it}_net"] = np.array([a.net_utility for a in agents])
        out[f"it{it}_gross"] = np.array([a.gross_utility for a in agents])
        out[f"it{it}_allocation_regret"] = np.array([float(a.get_allocation_regret()) for a in agents])
        out[f"it{it}_estimation_regret"] = np.array([float(a.get_estimation_regret()) for a in agents])
        out[f"it{it}_overbid_regret"] = np.array([float(a.get_overbid_regret()) for a in agents])
        out[f"it{it}_underbid_regret"] = np.array([float(a.get_underbid_regret()) for a in agents])
        out[f"it{it}_n_logs"] = np.array([len(a.logs) for a in agents])
        out[f"it{it}_pg0"] = np.array([float(getattr(a.bidder, "prev_gamma", np.nan)) for a in agents])
        for i, a in enumerate(agents):
            if is_ts[i]:
                seen = []
                upd = a.allocator.update

                def rec(contexts, items, outcomes, *rest, _upd=upd, _seen=seen, **kw):
                    _seen.append((np.array(contexts), np.array(items), np.array(outcomes)))
                    return _upd(contexts, items, outcomes, *rest, **kw)

                a.allocator.update = rec
                a.update(iteration=it)
                a.allocator.update = upd
                (cx, im, oc), = seen
                out[f"it{it}_a{i}_x"] = cx.astype(np.float32)
                out[f"it{it}_a{i}_item"] = im.astype(np.int32)
                out[f"it{it}_a{i}_outcome"] = oc.astype(np.uint8)
            else:
                a.update(iteration=it)
            a.clear_utility()
            a.clear_logs()
        out[f"it{it}_pg1"] = np.array([float(getattr(a.bidder, "prev_gamma", np.nan)) for a in agents])
        auction.clear_revenue()
        print(name, "iteration", it, "revenue", float(out[f"it{it}_revenue"]), out[f"it{it}_pg1"], flush=True)
    assert two_learners > 0 and overwritten > 0 and n_ge_p > 0  # the cases the collectors can get wrong
    meta = dict(N=N, P=P, E=E, OE=OE, max_slots=S, iters=ITERS, rounds=ROUNDS, allocation=config["allocation"],
                torch_seed=torch_seed, allocators=[type(a.allocator).__name__ for a in agents],
                bidders=[type(a.bidder).__name__ for a in agents], two_learner_rounds=int(two_learners),
                overwritten_prices=int(overwritten), rounds_n_ge_p=int(n_ge_p), config=cfg)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 1 << 20, f"{name}.npz is larger than 1 MiB"
    with open(os.path.join(OUT, name + ".json"), "w") as f:
        json.dump({"meta": meta}, f, indent=1)
    print("wrote", name, os.path.getsize(path), "bytes")


def main():
    MG.install_shims()
    cfg = MG.oracle_truthful_cfg(6, 12, 3, "FirstPrice", seed=3)
    cfg["agents"][0]["bidder"] = {"type": "EmpiricalShadedBidder", "kwargs": {"gamma_sigma": 0.05, "init_gamma": 0.9}}
    capture_update(cfg, "slots_update_fp_empirical")
    capture_update(MG.load_cfg("SP_Truthful_TS.json", num_participants_per_round=3, random_seed=3), "slots_update_sp_ts")


if __name__ == "__main__":
    main()
