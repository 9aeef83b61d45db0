"""Learners on multi-slot rounds: ag_lrts_collect_slots, ag_shading_collect_slots and
Auction(max_slots > 1, learners_on_slots=True).

The collectors are pure functions of the arrays they are handed, so the reference is the plain numpy
statement tests/slots_records_reference.py on host copies of exactly those arrays: every field of
every record, bit for bit, the count exact (nothing in a collector rounds). The statement itself is
pinned to the reference's own logs by tests/test_slots_records_reference.py, and the fixture tests
here check the GPU records against those logs directly as well.
"""
import json
import os
from collections import Counter

import numpy as np
import pytest

import slots_records_reference as RR
import test_gpu_trainer_branches as tb
from conftest import GOLDEN, mech_code, pop_args
from slots_cases import capture
from test_gpu_collect import (FIELDS, PACKED, PER_FIELD, _assert_records, _guarded, _host_out, _lrts_rows,
                              _lrts_store_rows, _records, expected_lrts_samples, expected_records)
from test_slots_records_reference import EMPIRICAL, TS, check_empirical_logs, check_lrts_logs

pytestmark = pytest.mark.gpu

BIG = (1 << 20) + 37  # one auction per lane: 4096 workgroups x 256 lanes = 2^20, then a second pass


# ---------------------------------------------------------------- helpers
def _catalogue(g, N, K, E):
    items = np.concatenate([g.normal(0, 1, (N, K, E)), -3.0 - g.random((N, K, 1))], axis=2)
    return items, g.lognormal(0.1, 0.2, (N, K))


def _rounds(g, N, P, E, B, S):
    """Contexts, P distinct participants, slot counts covering 1..S, the consumed doubles [B][min(S, P)]."""
    ctx = g.normal(0, 1, (B, E))
    part = np.ascontiguousarray(np.argsort(g.random((B, N)), axis=1)[:, :P].astype(np.int32))
    ns = g.integers(1, S + 1, B).astype(np.int32)
    if B >= S:
        ns[:S] = np.arange(1, S + 1)
    us = g.random((B, min(S, P)))
    return ctx, part, ns, us


def mixed(seed, P, S, mech, B, N=10, K=12, E=5, OE=4):
    """The mixed population of tests/test_gpu_slots.py: LR-TS sampling allocators beside Oracle ones;
    EmpiricalShaded (1, 7), an uninitialised (2) and two fitted (3, 8) DoublyRobust, a ValueLearning
    bidder bidding by search (4), a fitted PolicyLearning (5), truthful ones. The population does not
    depend on B (it is drawn before the rounds)."""
    from auctiongym_amd import _lib
    g = np.random.default_rng(seed)
    Do = OE + 1
    pop = dict(N=N, P=P, S=S, K=K, E=E, OE=OE, mech=mech)
    pop["items"], pop["values"] = _catalogue(g, N, K, E)
    pop["ak"] = ak = np.array([i % 2 for i in range(N)], np.int32)
    pop["bk"] = bk = np.resize(np.array([0, 1, 4, 4, 2, 3, 0, 1, 4, 0], np.int32), N)
    pop["init"] = np.resize(np.array([0, 0, 0, 1, 2, 1, 0, 0, 1, 0], np.int32), N)
    pop["modes"] = np.where(bk == _lib.BIDDER_VALUE_LEARNING, _lib.VL_SEARCH, _lib.VL_POLICY).astype(np.int32)
    pop["pg"], pop["gs"] = pg, gs = 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N)
    pop["m"] = g.normal(0, 1, (N, K, Do)).astype(np.float32)
    pop["q"] = q = (1.0 + 3.0 * g.random((N, K, Do))).astype(np.float32)
    pop["state"] = g.normal(0, 0.7, (N, 16)).astype(np.float32)
    ctx, part, ns, us = _rounds(g, N, P, E, B, S)
    z = g.normal(0, 1, (B, P, K, Do)) / np.sqrt(q[part])
    more = {"ts_noise": np.where((ak[part] == 1)[:, :, None, None], z, 0.0).astype(np.float32),
            "gamma_raw": g.normal(pg[part], gs[part]), "policy_eps": g.normal(0, 1, (B, P)).astype(np.float32),
            "gamma_grid": g.uniform(0.1, 1.0, (B, P, 128))}
    return pop, (ctx, part, ns, us, more)


def engine_of(pop, max_slots=None):
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(pop["N"], pop["P"], pop["K"], pop["E"], pop["OE"], pop["mech"], 1.0,
                        max_slots=pop["S"] if max_slots is None else max_slots)
    eng.set_agent_params(pop["ak"], pop["bk"], pop["pg"], pop["gs"])
    eng.load_catalog(pop["items"], pop["values"])
    eng.load_lrts(pop["m"], pop["q"], thompson_sampling=True)
    eng.set_dr_state(pop["state"], pop["init"])
    eng.set_bidder_modes(pop["modes"])
    return eng


def _upload(eng, ctx, part, ns, us, more):
    import torch
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(eng.device)  # noqa: E731
    inp = {"ctx": up(ctx.T), "part": up(part.T.astype(np.int32))}
    for k in ("gamma_raw", "policy_eps"):
        if more.get(k) is not None:
            inp[k] = up(more[k].T)
    if more.get("ts_noise") is not None:
        inp["ts_noise"] = up(eng.tile_ts_noise(more["ts_noise"]))
    if more.get("gamma_grid") is not None:
        inp["gamma_grid"] = up(more["gamma_grid"].transpose(1, 2, 0))
    return inp, up(ns.astype(np.int32)), up(us.T)


def _slot_host(out):
    """Device ag_slots_out arrays -> row-major host arrays ([B][P], [B][S], [B])."""
    return {k: (np.ascontiguousarray(v.cpu().numpy().T) if v.dim() == 2 else v.cpu().numpy()) for k, v in out.items()}


def _simulate(eng, ctx, part, ns, us, more):
    inp, dns, dus = _upload(eng, ctx, part, ns, us, more)
    out = eng.alloc_slot_outputs(len(ns))
    eng.simulate_slots(inp, dns, dus, out)
    return inp, out


def _collect(eng, inp, out, first=0, lrts=None, shading=None):
    """Both collectors on one simulated batch into the given (or fresh, exactly bounded) stores."""
    import torch
    B = inp["part"].shape[1]
    lrts = eng.new_lrts_samples(max(1, B * min(eng.max_slots, max(eng.P - 1, 0)))) if lrts is None else lrts
    shading = eng.new_shading_samples(B * eng.P, learning=True) if shading is None else shading
    eng.lrts_collect_slots(inp, out, lrts)
    eng.shading_collect_slots(inp, out, shading, first_auction=first)
    torch.cuda.synchronize()
    return lrts, shading


def _check(eng, pop, ctx, part, ns, us, more, what, first=0):
    """Simulate, collect, compare both stores with the statement on the device's outputs."""
    inp, out = _simulate(eng, ctx, part, ns, us, more)
    lrts, shading = _collect(eng, inp, out, first)
    o = _slot_host(out)
    want = RR.expected_records_slots(part, o, pop["bk"], pop["values"], pop["P"], first)
    assert len(want["order"]) == int((pop["bk"][part] != 0).sum())
    _assert_records(_records(shading), want, what)
    key, x = RR.expected_lrts_samples_slots(ctx, part, o, pop["ak"], pop["OE"], pop["P"])
    assert int(lrts["count"].item()) == len(key), what
    assert np.array_equal(_lrts_store_rows(lrts), _lrts_rows(key, x)), what
    return o, want, key


# ---------------------------------------------------------------- 1. the reference's own runs
@pytest.mark.parametrize("name", [EMPIRICAL, TS])
def test_fixture_records(gpu, name):
    """The fixture's rounds through ag_simulate_slots, collected in two flushes (first_auction 0 and
    512): the records equal the statement on the device's outputs and, through it and directly, the
    reference's own logs -- all 64 bits of order included."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    d, meta, _ = capture(name)
    S, N, P, R = meta["max_slots"], meta["N"], meta["P"], meta["rounds"]
    pa = pop_args(d, meta)
    eng = AuctionEngine(N, P, meta["K"], meta["E"], meta["OE"], mech_code(meta), 1.0, max_slots=S)
    eng.set_agent_params(pa["alloc_kind"], pa["bid_kind"], pa["prev_gamma"], pa["gamma_sigma"])
    eng.load_catalog(d["items"], d["values"])
    if "ts_m" in d:
        eng.load_lrts(d["ts_m"], d["ts_q"], thompson_sampling=True)
    lrts, shading = eng.new_lrts_samples(R * min(S, P - 1)), eng.new_shading_samples(R * P, learning=True)
    outs = []
    for lo, hi in ((0, 512), (512, R)):
        more = {"ts_noise": d["ts_noise"][lo:hi] if "ts_m" in d else None,
                "gamma_raw": d["gamma_raw"][lo:hi] if eng.shading else None}
        inp, out = _simulate(eng, d["ctx"][lo:hi], d["part"][lo:hi], d["num_slots"][lo:hi], d["u_slots"][lo:hi], more)
        _collect(eng, inp, out, lo, lrts, shading)
        outs.append(_slot_host(out))
    torch.cuda.synchronize()
    o = {k: np.concatenate([h[k] for h in outs]) for k in outs[0]}
    if not eng.shading:
        o["gamma"] = o["propensity"] = np.full((R, P), np.nan)
    want = RR.expected_records_slots(d["part"], o, pa["bid_kind"], d["values"], P, 0)
    key, x = RR.expected_lrts_samples_slots(d["ctx"], d["part"], o, pa["alloc_kind"], meta["OE"], P)
    assert int(shading["count"].item()) == len(want["order"]) and int(lrts["count"].item()) == len(key)
    if name == EMPIRICAL:
        got = _records(shading)
        _assert_records(got, want, name)
        check_empirical_logs(got, name, "GPU")
        assert len(key) == 0
    else:
        assert np.array_equal(_lrts_store_rows(lrts), _lrts_rows(key, x))
        n = len(key)
        check_lrts_logs(lrts["key"][:n].cpu().numpy().view(np.uint32), lrts["x"][:, :n].cpu().numpy().T, name, "GPU")
        assert len(want["order"]) == 0
    eng.close()


# ---------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("P", [1, 2, 3, 9])
def test_shapes(gpu, P, S, mech):
    """The mixed population at B = 1, 63, 65 (around a wave) and 1000 (four workgroups, a ragged
    tail), slot counts drawn, all 1 and all max_slots: P = 1 (F = 0: no LR-TS record, every utility
    +0.0, no NaN stored), n >= P, several records per lane."""
    seed = 8000 + 40 * P + 4 * S + mech
    eng = None
    for B in (1, 63, 65, 1000):
        pop, (ctx, part, ns, us, more) = mixed(seed, P, S, mech, B)
        eng = eng or engine_of(pop)
        for how, n in (("drawn", ns), ("one", np.ones(B, np.int32)), ("max", np.full(B, S, np.int32))):
            o, want, key = _check(eng, pop, ctx, part, n, us, more, (P, S, mech, B, how))
            assert np.array_equal(o["num_filled"], np.minimum(n, P - 1))
            if P == 1:
                assert len(key) == 0 and not want["won"].any()
                assert not want["utility"].view(np.uint64).any() and np.isnan(o["log_price"]).all()
            elif B == 1000:
                assert want["won"].any() and (want["utility"] != 0).any() and len(key) > 0
                lr_won = ((o["won_slot"] >= 0) & (pop["ak"][part] == 1)).sum(axis=1)
                assert len(key) == int(lr_won.sum())
                if how == "max" and min(S, P - 1) >= 2:
                    assert (lr_won >= 2).any()  # a lane with several records
                if how == "drawn" and S >= P:
                    assert (n >= P).any()
    eng.close()


def test_one_lane_owns_every_record_of_its_wave(gpu):
    """Hand-made outputs, no simulate: P = 9, max_slots = 8, 18 agents of which 0..8 are LR-TS
    allocators with EmpiricalShaded bidders. In every wave of 64 auctions one lane's auction has the
    nine learners (8 filled slots: 8 LR-TS records and 9 shading records of one lane) and its
    neighbours none at all; then 70 rows of a random mixture."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    N, P, S, K, E, OE, B = 18, 9, 8, 12, 5, 4, 3 * 64 + 70
    g = np.random.default_rng(8500)
    ak = np.array([1] * 9 + [0] * 9, np.int32)
    bk = ak.copy()
    items, values = _catalogue(g, N, K, E)
    eng = AuctionEngine(N, P, K, E, OE, 0, 1.0, max_slots=S)
    eng.set_agent_params(ak, bk, np.ones(N), np.full(N, 0.05))
    eng.load_catalog(items, values)
    part = np.tile(np.arange(9, 18, dtype=np.int32), (B, 1))
    owners = np.array([5, 64 + 63, 128])
    part[owners] = np.arange(9, dtype=np.int32)
    part[192:] = np.argsort(g.random((70, N)), axis=1)[:, :P]
    F = np.zeros(B, np.int32)
    F[owners] = 8
    F[192:] = g.integers(0, 9, 70)
    rank = np.argsort(g.random((B, P)), axis=1).astype(np.int32)  # rank[i][k]: the participant slot in slot k
    winner = np.where(np.arange(S)[None, :] < F[:, None], rank[:, :S], -1).astype(np.int32)
    won_slot = np.full((B, P), -1, np.int8)
    for k in range(S):
        rows = np.flatnonzero(F > k)
        won_slot[rows, winner[rows, k]] = k
    o = dict(winner=winner, outcome=((g.random((B, S)) < 0.5) & (winner >= 0)).astype(np.uint8), num_filled=F,
             log_price=np.where(F > 0, g.uniform(0.1, 2.5, B), np.nan), won_slot=won_slot,
             item=g.integers(0, K, (B, P)).astype(np.int32), gamma=g.uniform(0, 1.2, (B, P)),
             est_ctr=g.random((B, P)), propensity=g.uniform(0.1, 9, (B, P)))
    ctx = g.normal(0, 1, (B, E))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    inp = {"ctx": up(ctx.T), "part": up(part.T)}
    out = {k: up(v.T if v.ndim == 2 else v) for k, v in o.items()}
    lrts, shading = _collect(eng, inp, out, first=11)
    want = RR.expected_records_slots(part, o, bk, values, P, 11)
    key, x = RR.expected_lrts_samples_slots(ctx, part, o, ak, OE, P)
    first_wave = want["order"] < np.uint64((11 + 64) * P)
    assert int(first_wave.sum()) == 9 and int(want["won"][first_wave].sum()) == 8
    assert len(key) >= 24 and len(want["order"]) >= 27
    _assert_records(_records(shading), want, "hand-made")
    assert int(lrts["count"].item()) == len(key)
    assert np.array_equal(_lrts_store_rows(lrts), _lrts_rows(key, x))
    eng.close()


# ---------------------------------------------------------------- 3. the second grid-stride pass
def test_second_grid_stride_pass(gpu):
    """B = 2^20 + 37 at P = 3, max_slots = 2: the launch is capped at 4096 workgroups of 256 lanes,
    so the last 37 auctions are a second pass of the grid-stride loop. Inputs drawn on the device;
    every record of both stores checked."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    N, P, S, B = 8, 3, 2, BIG
    g = np.random.default_rng(8600)
    ak = np.array([i % 2 for i in range(N)], np.int32)
    bk = np.array([1, 1, 0, 0, 0, 0, 0, 0], np.int32)
    items, values = _catalogue(g, N, 12, 5)
    eng = AuctionEngine(N, P, 12, 5, 4, 0, 1.0, max_slots=S)
    eng.set_agent_params(ak, bk, 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N))
    eng.load_catalog(items, values)
    eng.load_lrts(g.normal(0, 1, (N, 12, 5)).astype(np.float32), np.ones((N, 12, 5), np.float32), thompson_sampling=False)
    inp = eng.alloc_inputs(B)
    assert "ts_noise" not in inp
    eng.generate(31, 0, inp)
    eng.generate_noise(31, 0, inp)
    tg = torch.Generator(device=eng.device).manual_seed(5)
    ns = torch.randint(1, S + 1, (B,), generator=tg, device=eng.device, dtype=torch.int32)
    us = torch.rand((S, B), generator=tg, device=eng.device, dtype=torch.float64)
    out = eng.alloc_slot_outputs(B)
    eng.simulate_slots(inp, ns, us, out)
    lrts, shading = _collect(eng, inp, out)
    o = _slot_host(out)
    ctx, part = inp["ctx"].cpu().numpy().T, np.ascontiguousarray(inp["part"].cpu().numpy().T)
    want = RR.expected_records_slots(part, o, bk, values, P, 0)
    key, x = RR.expected_lrts_samples_slots(ctx, part, o, ak, 4, P)
    assert (want["order"] >= np.uint64((1 << 20) * P)).any()  # the second pass has records of both kinds
    assert ((o["won_slot"][1 << 20:] >= 0) & (ak[part[1 << 20:]] == 1)).any()
    _assert_records(_records(shading), want, "second pass")
    assert int(lrts["count"].item()) == len(key) > B // 4
    assert np.array_equal(_lrts_store_rows(lrts), _lrts_rows(key, x))
    eng.close()


# ---------------------------------------------------------------- 4. two flushes, overflow
def test_two_flushes_into_one_store(gpu):
    """Two consecutive collects into one store, first_auction 2^33 + 5 and 2^33 + 5 + 600."""
    P, S, B, first = 3, 3, 1000, (1 << 33) + 5
    pop, (ctx, part, ns, us, more) = mixed(8700, P, S, 0, B)
    eng = engine_of(pop)
    lrts, shading = eng.new_lrts_samples(B * 2), eng.new_shading_samples(B * P, learning=True)
    wants, keys, xs = [], [], []
    for lo, hi in ((0, 600), (600, B)):
        sl = {k: v[lo:hi] for k, v in more.items()}
        inp, out = _simulate(eng, ctx[lo:hi], part[lo:hi], ns[lo:hi], us[lo:hi], sl)
        _collect(eng, inp, out, first + lo, lrts, shading)
        o = _slot_host(out)
        wants.append(RR.expected_records_slots(part[lo:hi], o, pop["bk"], pop["values"], P, first + lo))
        k, x = RR.expected_lrts_samples_slots(ctx[lo:hi], part[lo:hi], o, pop["ak"], pop["OE"], P)
        keys.append(k)
        xs.append(x)
    want = {f: np.concatenate([w[f] for w in wants]) for f in wants[0]}
    assert int(want["order"].min()) >= first * P > 1 << 34
    _assert_records(_records(shading), want, "two flushes")
    assert int(lrts["count"].item()) == sum(map(len, keys))
    assert np.array_equal(_lrts_store_rows(lrts), _lrts_rows(np.concatenate(keys), np.concatenate(xs)))
    eng.close()


def test_overflow_stays_inside_the_stores(gpu):
    """Stores 37 records too small inside sentinel-guarded allocations: count still counts every
    record, what fitted is a sub-multiset of the expected records, no guard element is touched, and
    the updates refuse the stores."""
    import torch
    P, S, B, G = 3, 3, 1000, 256
    pop, (ctx, part, ns, us, more) = mixed(8800, P, S, 1, B)
    eng = engine_of(pop)
    inp, out = _simulate(eng, ctx, part, ns, us, more)
    o = _slot_host(out)
    want = RR.expected_records_slots(part, o, pop["bk"], pop["values"], P, 0)
    key, x = RR.expected_lrts_samples_slots(ctx, part, o, pop["ak"], pop["OE"], P)
    R, RL = len(want["order"]), len(key)
    C, CL = R - 37, RL - 37
    assert C > 256 and CL > 256
    sent = {"agent": -7, "won": 0xAB, "order": -99}
    dt = {"agent": torch.int32, "won": torch.uint8, "order": torch.int64}
    st, guards = {"count": torch.zeros(1, dtype=torch.int64, device=eng.device)}, {}
    for f in FIELDS:
        st[f], guards[f] = _guarded((C,), dt.get(f, torch.float64), sent.get(f, -12345.678), G, eng.device)
    kview, kguard = _guarded((CL,), torch.int32, -7, G, eng.device)
    xview, xguard = _guarded((pop["OE"] + 1, CL), torch.float32, -12345.5, G, eng.device)
    small = {"key": kview, "x": xview, "count": torch.zeros(1, dtype=torch.int64, device=eng.device)}
    _collect(eng, inp, out, 0, small, st)
    assert int(st["count"].item()) == R and int(small["count"].item()) == RL
    for f in FIELDS:
        assert bool((guards[f] == sent.get(f, -12345.678)).all()), f
    assert bool((kguard == -7).all()) and bool((xguard == -12345.5).all())
    got = _records(st, C)
    assert len(np.unique(got["order"])) == C and np.isin(got["order"], want["order"]).all()
    kept = np.isin(want["order"], got["order"])
    _assert_records(got, {f: v[kept] for f, v in want.items()}, "the records that fitted")
    rows = lambda r: Counter(map(bytes, r))  # noqa: E731
    fitted, all_rows = rows(_lrts_store_rows(small, CL)), rows(_lrts_rows(key, x))
    assert sum(fitted.values()) == CL and not fitted - all_rows
    for call in (lambda: eng.empirical_update(st), lambda: eng.shading_counts(st),
                 lambda: eng.bidder_update(st, None, np.zeros(pop["N"], np.int64), 0), lambda: eng.lrts_update(small)):
        with pytest.raises(ValueError, match="overflow"):
            call()
    eng.close()


# ---------------------------------------------------------------- 5. one slot: the one-slot collectors' records
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("P", [2, 12])
def test_one_slot_context_equals_the_one_slot_collectors(gpu, P, mech):
    """max_slots = 1: *_collect_slots on ag_simulate_slots' outputs give the multiset of records
    *_collect give on ag_simulate's outputs of the same inputs, from per-field outputs and from the
    winner | outcome word."""
    import torch
    B = 1000
    pop, (ctx, part, ns, us, more) = mixed(8900 + 2 * P + mech, P, 1, mech, B, N=max(10, P))
    eng = engine_of(pop)
    assert (ns == 1).all() and us.shape == (B, 1)
    inp, out = _simulate(eng, ctx, part, ns, us, more)
    lrts, shading = _collect(eng, inp, out, first=3)
    got, got_rows = _records(shading), _lrts_store_rows(lrts)
    assert len(got["order"]) > 0 and len(got_rows) > 0
    inp1 = dict(inp, u=torch.from_numpy(np.ascontiguousarray(us[:, 0])).to(eng.device))
    for fields in (PER_FIELD, PACKED):
        o1 = eng.alloc_outputs(B, fields)
        eng.simulate(inp1, o1)
        l1, s1 = eng.new_lrts_samples(B), eng.new_shading_samples(B * P, learning=True)
        eng.lrts_collect(inp1, o1, l1)
        eng.shading_collect(inp1, o1, s1, first_auction=3)
        torch.cuda.synchronize()
        one = _records(s1)
        _assert_records(got, {f: one[f][np.argsort(one["order"], kind="stable")] for f in FIELDS}, (P, mech, fields[0]))
        assert np.array_equal(got_rows, _lrts_store_rows(l1)), (P, mech, fields[0])
        h = _host_out(o1)  # ... which are the one-slot statements' (tests/test_gpu_collect.py)
        _assert_records(got, expected_records(part, h, pop["bk"], pop["values"], P, 3), "one-slot statement")
        assert np.array_equal(got_rows, _lrts_rows(*expected_lrts_samples(ctx, part, h, pop["ak"], pop["OE"], P)))
    eng.close()


# ---------------------------------------------------------------- 6. updates from multi-slot stores
UPDATE_SEED, UPDATE_B = 9100, 1000


def _stated(seed=UPDATE_SEED, mech=0, B=UPDATE_B):
    """The mixed population at P = 3, max_slots = 3 simulated and collected -> (engine, population,
    stores, the stated shading records sorted by order, the stated LR-TS samples). ~300 records per
    agent."""
    pop, (ctx, part, ns, us, more) = mixed(seed, 3, 3, mech, B)
    eng = engine_of(pop)
    inp, out = _simulate(eng, ctx, part, ns, us, more)
    lrts, shading = _collect(eng, inp, out)
    o = _slot_host(out)
    want = RR.expected_records_slots(part, o, pop["bk"], pop["values"], pop["P"], 0)
    key, x = RR.expected_lrts_samples_slots(ctx, part, o, pop["ak"], pop["OE"], pop["P"])
    _assert_records(_records(shading), want, "update stores")
    assert np.array_equal(_lrts_store_rows(lrts), _lrts_rows(key, x))
    for a in np.flatnonzero(pop["bk"] != 0):  # a degenerate draw fails here, loudly
        sel = want["agent"] == a
        assert int(sel.sum()) <= 2000 and int(want["won"][sel].sum()) >= 2, a
        gm = want["gamma"][sel]
        assert (gm.max() - gm.min()) // 0.005 >= 2, a  # more than one gamma bucket
    for a in np.flatnonzero(pop["ak"] == 1):
        assert 2 <= int(((key >> 16) == a).sum()) <= 2000, a
    return eng, pop, lrts, shading, want, (key, x)


def test_lrts_update_from_a_multi_slot_store(gpu, oracle):
    """ag_lrts_update on the collected store == ora_lrts_update on the stated samples: epochs, every
    epoch's loss, m, q, prev_m, bit for bit."""
    eng, pop, lrts, _, _, (key, x) = _stated()
    ep, tr = eng.lrts_update(lrts, trace=True)
    tr = tr.cpu().numpy()
    m, q, pm = eng.lrts_state()
    for a in np.flatnonzero(pop["ak"] == 1):
        sel = (key >> 16) == a
        om, opm, oq, oep, oL = oracle.lrts_update(x[sel], (key[sel] >> 1) & 0x7FFF, key[sel] & 1, pop["m"][a], pop["m"][a],
                                                  pop["q"][a])
        assert ep[a] == oep > 0, a
        assert np.array_equal(tr[a, :oep], oL.astype(np.float32)), a
        assert np.array_equal(m[a], om) and np.array_equal(q[a], oq) and np.array_equal(pm[a], opm), a
    eng.close()


def test_empirical_update_from_a_multi_slot_store(gpu, oracle):
    """ag_empirical_update on the collected store == ora_empirical_update on the stated records."""
    eng, pop, _, shading, want, _ = _stated()
    pg = eng.empirical_update(shading)
    emp = np.flatnonzero(pop["bk"] == 1)
    assert len(emp) == 2
    for a in emp:
        sel = want["agent"] == a
        assert pg[a] == oracle.empirical_update(want["gamma"][sel], want["utility"][sel]) != pop["pg"][a], a
    rest = np.setdiff1d(np.arange(pop["N"]), emp)
    assert np.array_equal(pg[rest], pop["pg"][rest])
    eng.close()


def test_bidder_update_from_a_multi_slot_store(gpu, oracle):
    """ag_bidder_update of the mixed population's learning bidders (an uninitialised and two fitted
    DoublyRobust, a ValueLearning bidder by search, a fitted PolicyLearning) on the collected store
    == the oracle's DR / VL / PL updates on the stated records in log order: epochs, every traced
    loss, the models, the flags (tests/test_gpu_trainer_branches.py's checks)."""
    from auctiongym_amd import _lib
    eng, pop, _, shading, want, _ = _stated()
    N = pop["N"]
    eng.set_fit_noise_seed(tb.SEED)
    ep, stat, tr = eng.bidder_update(shading, None, np.zeros(N, np.int64), 0, trace=True)
    state, ini = eng.dr_state()
    got = dict(ep=ep, stat=stat, tr=tr.cpu().numpy(), state=state, ini=ini, mask=np.ones(N, np.int32))
    kinds = {v: k for k, v in tb.KINDS.items()}
    recs = {f: {} for f in FIELDS}
    learners = {}
    for a in np.flatnonzero(np.isin(pop["bk"], list(kinds))):
        sel = want["agent"] == a
        assert np.all(np.diff(want["order"][sel].astype(np.int64)) > 0)  # log order
        for f in FIELDS:
            recs[f][a] = want[f][sel]
        kind = kinds[int(pop["bk"][a])]
        mode = {"ips": tb.LOSSES[pop["modes"][a]], "dr": None,
                "dm": "search" if pop["modes"][a] == _lib.VL_SEARCH else "policy"}[kind]
        learners[a] = tb.learner(kind, int(a), n=int(sel.sum()), init=int(pop["init"][a]), mode=mode, src="slots")
    assert sorted(c["kind"] for c in learners.values()) == ["dm", "dr", "dr", "dr", "ips"]
    for a, c in learners.items():
        tb._check_agent(c, a, got, pop["state"], tb._oracle_fit(oracle, c, a, pop["state"], recs, ep[a, 2]))
    eng.close()


# ---------------------------------------------------------------- 7. missing arrays
def test_missing_arrays_are_named(gpu):
    pop, (ctx, part, ns, us, more) = mixed(9200, 3, 3, 0, 65)
    eng = engine_of(pop)
    inp, out = _simulate(eng, ctx, part, ns, us, more)
    lrts, shading = eng.new_lrts_samples(256), eng.new_shading_samples(256, learning=True)
    for where, name in (("in", "ctx"), ("in", "part"), ("out", "winner"), ("out", "outcome"), ("out", "num_filled"),
                        ("out", "item")):
        i = {k: v for k, v in inp.items() if where != "in" or k != name}
        o = {k: v for k, v in out.items() if where != "out" or k != name}
        with pytest.raises(ValueError, match=rf"ag_lrts_collect_slots: needs .*{where}\.{name}"):
            eng.lrts_collect_slots(i, o, lrts)
    for where, name in (("in", "part"), ("out", "won_slot"), ("out", "log_price"), ("out", "outcome"), ("out", "item"),
                        ("out", "gamma"), ("out", "est_ctr"), ("out", "propensity")):
        i = {k: v for k, v in inp.items() if where != "in" or k != name}
        o = {k: v for k, v in out.items() if where != "out" or k != name}
        with pytest.raises(ValueError, match=rf"ag_shading_collect_slots: .*{where}\.{name}"):
            eng.shading_collect_slots(i, o, shading)
    small = eng.new_shading_samples(256)  # without ctr / propensity: est_ctr and propensity are not needed
    eng.shading_collect_slots(inp, {k: v for k, v in out.items() if k not in ("est_ctr", "propensity")}, small)
    import torch
    torch.cuda.synchronize()
    assert int(small["count"].item()) == int((pop["bk"][part] != 0).sum())
    assert int(lrts["count"].item()) == 0 and int(shading["count"].item()) == 0
    eng.close()


# ---------------------------------------------------------------- 8. Auction(learners_on_slots=True)
def _update_capture(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)["meta"]
    return np.load(os.path.join(GOLDEN, name + ".npz")), meta


def _auction(meta, tmp_path, **kw):
    import auctiongym_amd.main as M
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(meta["config"]))
    rng, config, agent_configs, a2i, a2v, _, _, E, var, OE = M.parse_config(str(p))
    agents = M.instantiate_agents(rng, agent_configs, a2v, a2i)
    auction, num_iter, rounds, _ = M.instantiate_auction(rng, config, a2i, a2v, agents, meta["max_slots"], E, var, OE, **kw)
    return rng, auction, num_iter, rounds


def _check_iteration(k, it, rng, auction):
    rt = dict(rtol=1e-9, atol=1e-9)
    ag = auction.agents
    np.testing.assert_allclose(auction.revenue, float(k[f"it{it}_revenue"]), **rt)
    np.testing.assert_allclose([a.net_utility for a in ag], k[f"it{it}_net"], **rt)
    np.testing.assert_allclose([a.gross_utility for a in ag], k[f"it{it}_gross"], **rt)
    np.testing.assert_allclose([a.get_allocation_regret() for a in ag], k[f"it{it}_allocation_regret"], **rt)
    np.testing.assert_allclose([a.get_estimation_regret() for a in ag], k[f"it{it}_estimation_regret"], **rt)
    np.testing.assert_allclose([a.get_overbid_regret() for a in ag], k[f"it{it}_overbid_regret"], **rt)
    np.testing.assert_allclose([a.get_underbid_regret() for a in ag], k[f"it{it}_underbid_regret"], **rt)
    st, after = rng.bit_generator.state, json.loads(str(k[f"it{it}_np_state"]))
    assert (str(st["state"]["state"]), str(st["state"]["inc"]), st["has_uint32"], st["uinteger"]) == \
        (after["state"], after["inc"], after["has_uint32"], after["uinteger"])


@pytest.mark.parametrize("how", ["batch", "rounds"])
def test_auction_dropin_empirical(gpu, tmp_path, how):
    """The reference's driver loop at max_slots = 3 on six EmpiricalShadedBidders over FirstPrice
    (tests/golden/make_golden_slots_update.py), through Auction(learners_on_slots=True): every
    iteration's prev_gamma before and after the updates bit for bit, utilities, regrets and revenue to
    1e-9, the numpy generator in the reference's state."""
    k, meta = _update_capture("slots_update_fp_empirical")
    assert meta["two_learner_rounds"] > 0 and meta["overwritten_prices"] > 0 and meta["rounds_n_ge_p"] > 0
    rng, auction, num_iter, rounds = _auction(meta, tmp_path, learners_on_slots=True)
    assert (num_iter, rounds, auction.max_slots) == (3, 1000, 3)
    for it in range(num_iter):
        if how == "batch":
            auction.simulate_batch(rounds)
        else:
            for _ in range(rounds):
                auction.simulate_opportunity()
        _check_iteration(k, it, rng, auction)
        assert [a.bidder.prev_gamma for a in auction.agents] == list(k[f"it{it}_pg0"])
        for a in auction.agents:
            a.update(iteration=it)
            a.clear_utility()
            a.clear_logs()
        assert [a.bidder.prev_gamma for a in auction.agents] == list(k[f"it{it}_pg1"]), it
        auction.clear_revenue()


@pytest.mark.parametrize("how", ["batch", "rounds"])
def test_auction_dropin_sp_truthful_ts(gpu, tmp_path, how):
    """SP_Truthful_TS at max_slots = 3: iteration 0 to 1e-9, each agent's collected won samples equal,
    as a multiset, to the inputs of the reference's first PyTorchLogisticRegressionAllocator.update;
    the later iterations run (the float32 torch fit is chaotic, PARITY.md: they are not compared).
    Per round (simulate_opportunity) the first iteration only."""
    import torch
    k, meta = _update_capture("slots_update_sp_ts")
    assert meta["two_learner_rounds"] > 0 and meta["overwritten_prices"] > 0 and meta["rounds_n_ge_p"] > 0
    torch.manual_seed(meta["torch_seed"])
    rng, auction, num_iter, rounds = _auction(meta, tmp_path, learners_on_slots=True)
    for it in range(num_iter if how == "batch" else 1):
        if how == "batch":
            auction.simulate_batch(rounds)
        else:
            for _ in range(rounds):
                auction.simulate_opportunity()
        if it == 0:
            _check_iteration(k, 0, rng, auction)
            auction._flush()
            st = auction._stores["lrts"]
            n = int(st["count"].item())
            key, x = st["key"][:n].cpu().numpy().view(np.uint32), st["x"][:, :n].cpu().numpy().T
            for i in range(meta["N"]):
                sel = (key >> 16) == i
                want_key = (np.uint32(i) << 16) | (k[f"it0_a{i}_item"].astype(np.uint32) << 1) | k[f"it0_a{i}_outcome"]
                assert int(sel.sum()) == len(want_key) >= 2, i
                assert np.array_equal(_lrts_rows(key[sel], x[sel]), _lrts_rows(want_key, k[f"it0_a{i}_x"])), i
        assert sum(a.num_logs() for a in auction.agents) == rounds * meta["P"]
        for a in auction.agents:
            a.update(iteration=it)
            a.clear_utility()
            a.clear_logs()
        assert all(a.allocator.epochs > 0 for a in auction.agents)
        auction.clear_revenue()


def test_default_still_refuses_and_memory_is_refused(gpu, tmp_path):
    """Without learners_on_slots the constructor raises as before, with the same message;
    Agent(memory > 0) with several slots is refused with a message of its own either way."""
    for name in ("slots_update_fp_empirical", "slots_update_sp_ts"):
        _, meta = _update_capture(name)
        with pytest.raises(NotImplementedError, match="log-fed updates from multi-slot rounds"):
            _auction(meta, tmp_path)
        with pytest.raises(NotImplementedError, match="log-fed updates from multi-slot rounds"):
            _auction(meta, tmp_path, learners_on_slots=False)
    cfg = json.loads(json.dumps(meta["config"]))
    for a in cfg["agents"]:
        a["memory"] = 100
    with pytest.raises(NotImplementedError, match=r"Agent\(memory > 0\): the records an agent keeps"):
        _auction(dict(meta, config=cfg), tmp_path, learners_on_slots=True)
    _, auction, _, _ = _auction(dict(meta, max_slots=1), tmp_path)  # one slot: as before
    assert auction.max_slots == 1
