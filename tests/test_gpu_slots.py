"""Multi-slot auctions on the GPU: ag_simulate_slots, ag_allocate_slots and Auction(max_slots > 1).

Expected results: the oracle's per-participant outputs (they do not depend on the number of slots)
plus tests/slots_reference.py (pinned to the reference's own multi-slot runs by
tests/test_slots_reference.py) -- bit for bit, every counter limb included.
"""
import json

import numpy as np
import pytest

import slots_reference as SR
from conftest import mech_code, pop_args
from counter_reference import limbs_of
from slots_cases import ORACLE_SLOT_CAPTURES, POP_SLOT_CAPTURES, SLOT_CAPTURES, capture, fixture_expected

pytestmark = pytest.mark.gpu

PER_PART = ("item", "bid", "est_ctr", "true_ctr", "best_ev")
PER_SLOT = ("winner", "price", "second_price", "outcome")


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
        ns[:S] = np.arange(1, S + 1)  # every n from 1 to max_slots, n >= P included
    us = g.random((B, min(S, P)))
    us[np.arange(min(S, P))[None, :] >= np.minimum(ns, P)[:, None]] = np.nan  # as the draw functions leave them
    return ctx, part, ns, us


def _upload(eng, ctx, part, ns, us, **more):
    import torch
    d = eng.device
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(d)  # noqa: E731  (a copy: fixtures are read-only)
    inp = {"ctx": up(ctx.T), "part": up(part.T.astype(np.int32))}
    for k in ("gamma_raw", "policy_eps"):
        if more.get(k) is not None:
            inp[k] = up(more[k].T)
    if more.get("ts_noise") is not None:
        inp["ts_noise"] = up(eng.tile_ts_noise(more["ts_noise"]))
    if more.get("gamma_grid") is not None:
        inp["gamma_grid"] = up(more["gamma_grid"].transpose(1, 2, 0))
    return inp, up(ns.astype(np.int32)), up(us.T)


def _run(eng, ctx, part, ns, us, more=None, fields=None, counters=True):
    """ag_simulate_slots -> row-major host arrays ([B][P], [B][S], [B]) and the counter limbs."""
    import torch
    inp, dns, dus = _upload(eng, ctx, part, ns, us, **(more or {}))
    B = len(ns)
    out = eng.alloc_slot_outputs(B, fields)
    for v in out.values():  # poison: what the kernel must write is visible
        v.fill_(77) if not v.dtype.is_floating_point else v.fill_(-7.5)
    cnt = eng.new_counters() if counters else None
    eng.simulate_slots(inp, dns, dus, out, cnt)
    torch.cuda.synchronize()
    o = {k: (v.cpu().numpy().T if v.dim() == 2 else v.cpu().numpy()) for k, v in out.items()}
    if counters:
        o["counters_fx"] = cnt.cpu().numpy()
    return o


def _expected(orc, mech, part, ns, us, S, N):
    return SR.simulate(mech, orc, part, ns, us, S, N=N)


def _compare(got, orc, exp, what, pop=False):
    for k in PER_PART + (("gamma", "propensity") if pop else ()):
        if k in got:
            assert np.array_equal(got[k], orc[k], equal_nan=True), f"{what}: {k}"
    for k in PER_SLOT + ("log_price", "num_filled", "won_slot"):
        if k in got:
            assert np.array_equal(got[k], exp[k], equal_nan=True), f"{what}: {k}"
    if "counters_fx" in got:
        assert np.array_equal(got["counters_fx"], np.array(limbs_of(exp["counters"]), np.int64)), f"{what}: counters"


def _oracle_engine(N, P, K, E, mech, items, values, S):
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(N, P, K, E, min(E, 4), mech, 1.0, max_slots=S)
    eng.load_catalog(items, values)
    return eng


def _u0(us):
    return np.nan_to_num(us[:, 0])


# ---------------------------------------------------------------- the reference's own runs
@pytest.mark.parametrize("B", [1, 1000])
@pytest.mark.parametrize("name", ORACLE_SLOT_CAPTURES)
def test_oracle_fixtures_replay(gpu, oracle, name, B):
    d, meta, _ = capture(name)
    mech, S, N, P = mech_code(meta), meta["max_slots"], meta["N"], meta["P"]
    eng = _oracle_engine(N, P, meta["K"], meta["E"], mech, d["items"], d["values"], S)
    sl = slice(0, B)
    got = _run(eng, d["ctx"][sl], d["part"][sl], d["num_slots"][sl], d["u_slots"][sl])
    eng.close()
    orc = oracle.simulate(mech, d["items"], d["values"], d["ctx"][sl], d["part"][sl], _u0(d["u_slots"][sl]))
    exp = _expected(orc, mech, d["part"][sl], d["num_slots"][sl], d["u_slots"][sl], S, N)
    _compare(got, orc, exp, f"{name} B={B}")
    # ... and the reference's log fields themselves
    full = fixture_expected(name)
    assert np.array_equal(got["bid"], d["slot_bid"][sl])
    assert np.array_equal(got["won_slot"] >= 0, d["won"][sl].astype(bool))
    assert np.array_equal(got["won_slot"], full["won_slot"][sl])
    lp = np.where(got["num_filled"] > 0, got["log_price"], 0.0)
    assert np.array_equal(np.broadcast_to(lp[:, None], (B, P)), d["slot_price"][sl])


@pytest.mark.parametrize("name", POP_SLOT_CAPTURES)
def test_population_fixtures_replay(gpu, oracle, name):
    from auctiongym_amd.engine import AuctionEngine
    d, meta, _ = capture(name)
    mech, S, N, P, B = mech_code(meta), meta["max_slots"], meta["N"], meta["P"], 1000
    pa = pop_args(d, meta)
    eng = AuctionEngine(N, P, meta["K"], meta["E"], meta["OE"], mech, 1.0, max_slots=S)
    eng.set_agent_params(pa["alloc_kind"], pa["bid_kind"], pa["prev_gamma"], pa["gamma_sigma"])
    eng.load_catalog(d["items"], d["values"])
    more = {}
    if "ts_m" in d:
        eng.load_lrts(d["ts_m"], d["ts_q"], thompson_sampling=True)
        more["ts_noise"] = d["ts_noise"][:B]
    if eng.shading:
        more["gamma_raw"] = d["gamma_raw"][:B]
    sl = slice(0, B)
    got = _run(eng, d["ctx"][sl], d["part"][sl], d["num_slots"][sl], d["u_slots"][sl], more)
    eng.close()
    pa = dict(pa, gamma_raw=d["gamma_raw"][sl], ts_noise=d["ts_noise"][sl] if "ts_noise" in d else None)
    orc = oracle.simulate_pop(mech, d["items"], d["values"], d["ctx"][sl], d["part"][sl], _u0(d["u_slots"][sl]), **pa)
    exp = _expected(orc, mech, d["part"][sl], d["num_slots"][sl], d["u_slots"][sl], S, N)
    _compare(got, orc, exp, name, pop=eng.shading)
    assert np.array_equal(got["bid"], d["slot_bid"][sl])
    assert np.array_equal(got["won_slot"], fixture_expected(name)["won_slot"][sl])


# ---------------------------------------------------------------- synthetic Oracle populations
@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("P", [1, 2, 3, 9, 17])
def test_synthetic_oracle_populations(gpu, oracle, P, S):
    """Both mechanisms, B = 1000 (a ragged last tile) and B = 1; D and K vary with the case; the exact
    item search on the odd cases."""
    for mech in (0, 1):
        n = P * 10 + S + mech
        D, K = (2, 6, 8)[n % 3], (3, 7, 12, 16)[n % 4]
        E, N = D - 1, 17 if P == 17 else P + 3
        g = np.random.default_rng(7000 + n)
        items, values = _catalogue(g, N, K, E)
        eng = _oracle_engine(N, P, K, E, mech, items, values, S)
        if n % 2:
            eng.set_item_search(True)
        for B in (1000, 1):
            ctx, part, ns, us = _rounds(g, N, P, E, B, S)
            if B > 1:
                assert set(np.unique(ns)) == set(range(1, S + 1)) and ((ns >= P).any() or S < P)
            got = _run(eng, ctx, part, ns, us)
            orc = oracle.simulate(mech, items, values, ctx, part, _u0(us))
            exp = _expected(orc, mech, part, ns, us, S, N)
            _compare(got, orc, exp, f"P={P} S={S} mech={mech} D={D} K={K} B={B}")
            assert np.array_equal(exp["num_filled"], np.minimum(ns, P - 1))
        eng.close()


# ---------------------------------------------------------------- a mixed population
def _mixed(seed, P, S, mech, B, N=10, K=12, E=5, OE=4):
    """LR-TS sampling allocators beside Oracle ones; EmpiricalShaded, an uninitialised and a fitted
    DoublyRobust, a ValueLearning bidder bidding by search, a fitted PolicyLearning, truthful ones."""
    from auctiongym_amd import _lib
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(seed)
    Do = OE + 1
    items, values = _catalogue(g, N, K, E)
    ak = np.array([i % 2 for i in range(N)], np.int32)
    bk = np.resize(np.array([0, 1, 4, 4, 2, 3, 0, 1, 4, 0], np.int32), N)
    init = np.resize(np.array([0, 0, 0, 1, 2, 1, 0, 0, 1, 0], np.int32), N)  # AG_LEARNER_*: agent 2 uninitialised, 3 fitted, 4 search
    modes = np.where(bk == _lib.BIDDER_VALUE_LEARNING, _lib.VL_SEARCH, _lib.VL_POLICY).astype(np.int32)
    pg, gs = 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N)
    m = g.normal(0, 1, (N, K, Do)).astype(np.float32)
    q = (1.0 + 3.0 * g.random((N, K, Do))).astype(np.float32)
    state = g.normal(0, 0.7, (N, 16)).astype(np.float32)
    ctx, part, ns, us = _rounds(g, N, P, E, B, S)
    z = g.normal(0, 1, (B, P, K, Do)) / np.sqrt(q[part])
    more = {"ts_noise": np.where((ak[part] == 1)[:, :, None, None], z, 0.0).astype(np.float32),
            "gamma_raw": g.normal(pg[part], gs[part]), "policy_eps": g.normal(0, 1, (B, P)).astype(np.float32),
            "gamma_grid": g.uniform(0.1, 1.0, (B, P, 128))}

    def engine(max_slots):
        eng = AuctionEngine(N, P, K, E, OE, mech, 1.0, max_slots=max_slots)
        eng.set_agent_params(ak, bk, pg, gs)
        eng.load_catalog(items, values)
        eng.load_lrts(m, q, thompson_sampling=True)
        eng.set_dr_state(state, init)
        eng.set_bidder_modes(modes)
        return eng

    orc = lambda O, u: O.simulate_pop(mech, items, values, ctx, part, u, ak, bk, pg, gs, OE=OE, ts_m=m,  # noqa: E731
                                      ts_noise=more["ts_noise"], gamma_raw=more["gamma_raw"], ts_sample=True,
                                      dr_state=state, dr_init=init, policy_eps=more["policy_eps"],
                                      gamma_grid=more["gamma_grid"])
    return engine, (ctx, part, ns, us, more), orc, N


@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("P", [3, 9])
def test_mixed_population(gpu, oracle, P, mech):
    for B in (1000, 1):
        engine, (ctx, part, ns, us, more), orc, N = _mixed(7300 + P * 2 + mech, P, 3, mech, B)
        eng = engine(3)
        got = _run(eng, ctx, part, ns, us, more)
        eng.close()
        o = orc(oracle, _u0(us))
        _compare(got, o, _expected(o, mech, part, ns, us, 3, N), f"mixed P={P} mech={mech} B={B}", pop=True)


# ---------------------------------------------------------------- ties, unfilled slots, NULL outputs
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("case", ["two_equal", "all_equal"])
def test_exact_ties_go_to_the_lower_participant_slot(gpu, oracle, case, mech):
    N, P, K, E, S = 6, 5, 7, 5, 3
    g = np.random.default_rng(7500 + mech)
    items, values = _catalogue(g, N, K, E)
    if case == "two_equal":
        items[4], values[4] = items[1], values[1]
    else:
        items[:], values[:] = items[0], values[0]
    eng = _oracle_engine(N, P, K, E, mech, items, values, S)
    for B in (1000, 1):
        ctx, part, ns, us = _rounds(g, N, P, E, B, S)
        if B == 1:
            # the two equal catalogues meet, every slot asked for
            part[0], ns[0], us[0] = (1, 4, 0, 2, 3), S, g.random(us.shape[1])
        got = _run(eng, ctx, part, ns, us)
        orc = oracle.simulate(mech, items, values, ctx, part, _u0(us))
        tied = (np.sort(orc["bid"], axis=1)[:, 1:] == np.sort(orc["bid"], axis=1)[:, :-1]).any(axis=1)
        assert tied.sum() > B // 2
        _compare(got, orc, _expected(orc, mech, part, ns, us, S, N), f"ties {case} B={B}")
        if case == "all_equal":  # the ranking is the participant order
            f = got["num_filled"]
            for k in range(S):
                assert (got["winner"][f > k, k] == k).all()
    eng.close()


@pytest.mark.parametrize("B", [1, 1000])
@pytest.mark.parametrize("mech", [0, 1])
def test_unfilled_slots_and_null_outputs(gpu, oracle, mech, B):
    """Unfilled slots hold -1 / NaN / 0 (P = 1: every slot, log_price NaN, nobody wins); arrays left
    NULL are skipped and the others, and the counters, do not change."""
    N, K, E, S = 5, 7, 5, 3
    g = np.random.default_rng(7600 + mech)
    items, values = _catalogue(g, N, K, E)
    for P in (1, 2):
        ctx, part, ns, us = _rounds(g, N, P, E, B, S)
        eng = _oracle_engine(N, P, K, E, mech, items, values, S)
        full = _run(eng, ctx, part, ns, us)
        F = np.minimum(ns, P - 1)
        unf = np.arange(S)[None, :] >= F[:, None]
        assert (full["winner"][unf] == -1).all() and np.isnan(full["price"][unf]).all()
        assert np.isnan(full["second_price"][unf]).all() and (full["outcome"][unf] == 0).all()
        assert np.isnan(full["log_price"][F == 0]).all() and np.array_equal(full["num_filled"], F)
        if P == 1:
            assert unf.all() and (full["won_slot"] == -1).all() and not full["counters_fx"][:, 10].any()  # N_WON
        some = _run(eng, ctx, part, ns, us, fields=("winner", "log_price", "bid", "won_slot"))
        assert set(some) == {"winner", "log_price", "bid", "won_slot", "counters_fx"}
        for k in some:
            assert np.array_equal(some[k], full[k], equal_nan=True), k
        none = _run(eng, ctx, part, ns, us, fields=())
        assert np.array_equal(none["counters_fx"], full["counters_fx"])
        nocnt = _run(eng, ctx, part, ns, us, counters=False)
        for k in nocnt:
            assert np.array_equal(nocnt[k], full[k], equal_nan=True), k
        eng.close()


# ---------------------------------------------------------------- launches and grids
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("pop", ["oracle", "mixed"])
def test_batch_split_and_grid_stride(gpu, oracle, pop, mech):
    """Three launches (AG_OPT_LAUNCH_AUCTIONS) and one workgroup per CU (a grid-stride pass per
    block when the batch has more tiles than CUs) give the same outputs and counter limbs."""
    S = 3
    if pop == "oracle":
        N, P, K, E, B = 8, 4, 7, 5, 1000
        g = np.random.default_rng(7700 + mech)
        items, values = _catalogue(g, N, K, E)
        ctx, part, ns, us = _rounds(g, N, P, E, B, S)
        more = None
        engine = lambda: _oracle_engine(N, P, K, E, mech, items, values, S)  # noqa: E731
    else:
        B = 1000
        mk, (ctx, part, ns, us, more), _, N = _mixed(7710 + mech, 3, S, mech, B)
        engine = lambda: mk(S)  # noqa: E731
    eng = engine()
    base = _run(eng, ctx, part, ns, us, more)
    eng.set_launch_auctions(400)
    split = _run(eng, ctx, part, ns, us, more)
    eng.set_launch_auctions(0)
    for k in base:
        assert np.array_equal(split[k], base[k], equal_nan=True), k
    if pop == "mixed":  # (its search grids are 3 KB per auction: the larger batch is the Oracle case's)
        eng.close()
        return
    eng.set_blocks_per_cu(1)
    # more tiles than CUs: blocks take a second grid-stride pass
    import torch
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    Bl = (cus + 3) * 256 + 11
    reps = -(-Bl // B)
    big = [np.concatenate([a] * reps)[:Bl] for a in (ctx, part, ns, us)]
    bmore = None if more is None else {k: np.concatenate([v] * reps)[:Bl] for k, v in more.items()}
    one = _run(eng, *big, bmore)
    eng.set_blocks_per_cu(0)
    ref = _run(eng, *big, bmore)
    eng.close()
    for k in base:
        assert np.array_equal(one[k], ref[k], equal_nan=True), k
    for k in base:
        if k != "counters_fx":
            assert np.array_equal(ref[k][:B], base[k], equal_nan=True), k


# ---------------------------------------------------------------- the pinned one-slot path
@pytest.mark.parametrize("B", [1, 1000])
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("P", [2, 12])
@pytest.mark.parametrize("pop", ["oracle", "mixed"])
def test_one_slot_context_equals_ag_simulate(gpu, pop, P, mech, B):
    """ag_simulate_slots on a num_slots = 1 context with u_slots = u: every output and counter limb of
    ag_simulate (k_oracle / the per-P builds / the runtime-P kernel), under both mechanisms -- under
    SecondPrice the OVERBID term the multi-slot build issues is exactly 0 and adds nothing."""
    import torch
    if pop == "oracle":
        N, K, E = 14, 12, 5
        g = np.random.default_rng(7800 + 2 * P + mech)
        items, values = _catalogue(g, N, K, E)
        ctx, part, ns, us = _rounds(g, N, P, E, B, 1)
        more = {}
        eng = _oracle_engine(N, P, K, E, mech, items, values, 1)
    else:
        mk, (ctx, part, ns, us, more), _, N = _mixed(7850 + 2 * P + mech, P, 1, mech, B, N=max(10, P))
        eng = mk(1)
    assert (ns == 1).all() and us.shape == (B, 1)
    got = _run(eng, ctx, part, ns, us, more)
    inp, _, dus = _upload(eng, ctx, part, ns, us, **more)
    inp["u"] = dus[0].contiguous()
    out = eng.alloc_outputs(B)
    cnt = eng.new_counters()
    eng.simulate(inp, out, cnt)
    torch.cuda.synchronize()
    eng.close()
    for k in PER_SLOT:
        assert np.array_equal(got[k][:, 0], out[k].cpu().numpy(), equal_nan=True), k
    for k in PER_PART + (("gamma", "propensity") if pop == "mixed" else ()):
        assert np.array_equal(got[k], out[k].cpu().numpy().T, equal_nan=True), k
    assert np.array_equal(got["log_price"], out["price"].cpu().numpy())
    assert np.array_equal(got["won_slot"] == 0, np.arange(P)[None, :] == out["winner"].cpu().numpy()[:, None])
    assert np.array_equal(got["counters_fx"], cnt.cpu().numpy())


# ---------------------------------------------------------------- ag_allocate_slots
@pytest.mark.parametrize("P", [1, 2, 16, 64])
def test_allocate_slots(gpu, P):
    import torch
    from auctiongym_amd.engine import AuctionEngine
    B = 1000
    g = np.random.default_rng(7900 + P)
    for mech in (0, 1):
        eng = AuctionEngine(P, P, 1, 1, 0, mech)
        for S in (1, 2, 3, 8):
            bids = g.lognormal(0, 1, (B, P))
            bids[::7, : max(1, P // 2)] = bids[::7, :1]  # exact ties
            ns = g.integers(1, S + 1, B).astype(np.int32)
            db = torch.from_numpy(np.ascontiguousarray(bids.T)).to(eng.device)
            w, p, s = (t.cpu().numpy().T for t in eng.allocate_slots(db, torch.from_numpy(ns).to(eng.device), S))
            ew, ep, es = SR.allocate_padded(mech, bids, ns, S)
            assert np.array_equal(w, ew) and np.array_equal(p, ep, equal_nan=True)
            assert np.array_equal(s, es, equal_nan=True)
            w2, _, _ = (t.cpu().numpy().T for t in eng.allocate_slots(db, None, S))  # NULL: max_slots everywhere
            assert np.array_equal(w2, SR.allocate_padded(mech, bids, np.full(B, S), S)[0])
        eng.close()


@pytest.mark.parametrize("name", SLOT_CAPTURES)
def test_allocate_slots_reproduces_the_reference(gpu, name):
    import torch
    from auctiongym_amd.AuctionAllocation import FirstPrice, SecondPrice
    d, meta, _ = capture(name)
    mechanism = (FirstPrice if mech_code(meta) == 0 else SecondPrice)()
    db = torch.from_numpy(np.array(d["slot_bid"].T, order="C")).cuda()
    w, p, s = mechanism.allocate_batch(db, torch.from_numpy(d["num_slots"].copy()))
    S = int(d["num_slots"].max())
    assert np.array_equal(w.cpu().numpy().T, d["alloc_winner"][:, :S])
    assert np.array_equal(p.cpu().numpy().T, d["alloc_price"][:, :S], equal_nan=True)
    assert np.array_equal(s.cpu().numpy().T, d["alloc_second"][:, :S], equal_nan=True)
    for r in (0, 1, 2, 3):  # the per-call form: the reference's ragged arrays
        n = int(d["num_slots"][r])
        ww, pp, ss = mechanism.allocate(d["slot_bid"][r], n)
        ew, ep, es = SR.allocate(mech_code(meta), d["slot_bid"][r], n)
        assert ww.dtype == np.int64 and ww.tolist() == ew and pp.tolist() == ep and ss.tolist() == es


def test_refusals(gpu):
    import torch
    from auctiongym_amd.engine import AuctionEngine
    with pytest.raises(NotImplementedError, match="num_slots"):
        AuctionEngine(6, 2, 12, 5, 4, 1, max_slots=9)
    with pytest.raises(ValueError, match="num_slots"):
        AuctionEngine(6, 2, 12, 5, 4, 1, max_slots=0)
    eng = AuctionEngine(70, 65, 1, 1, 0, 0)
    with pytest.raises(NotImplementedError, match="P = 65 > 64"):
        eng.allocate_slots(torch.zeros((65, 4), dtype=torch.float64, device=eng.device), None, 2)
    eng.close()
    g = np.random.default_rng(1)
    items, values = _catalogue(g, 6, 12, 5)
    eng = _oracle_engine(6, 2, 12, 5, 1, items, values, 2)
    B = 8
    inp = eng.alloc_inputs(B)
    eng.generate(0, 0, inp)
    with pytest.raises(NotImplementedError, match="ag_simulate_slots"):
        eng.simulate(inp, eng.alloc_outputs(B))
    with pytest.raises(NotImplementedError, match="ag_simulate_slots"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(B))
    with pytest.raises(NotImplementedError, match="ag_simulate_slots"):
        eng.lrts_collect(inp, eng.alloc_outputs(B), eng.new_lrts_samples(16))
    with pytest.raises(NotImplementedError, match="ag_simulate_slots"):
        eng.shading_collect(inp, eng.alloc_outputs(B, ("winner", "price", "outcome", "item", "gamma")),
                            eng.new_shading_samples(16))
    eng.close()


# ---------------------------------------------------------------- Auction(max_slots > 1)
def _auction(meta, tmp_path, max_slots):
    import auctiongym_amd.main as M
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(meta["config"]))
    rng, config, agent_configs, a2i, a2v, _, _, E, var, OE = M.parse_config(str(p))
    agents = M.instantiate_agents(rng, agent_configs, a2v, a2i)
    auction, *_ = M.instantiate_auction(rng, config, a2i, a2v, agents, max_slots, E, var, OE)
    return rng, auction


@pytest.mark.parametrize("how", ["batch", "rounds"])
@pytest.mark.parametrize("name", ["slots_fp_oracle_p4_s3", "slots_sp_oracle_p4_s3"])
def test_auction_dropin(gpu, name, how, tmp_path):
    """Auction(max_slots = 3) built as main.py builds it from the fixture's config: utilities,
    regrets and revenue of the reference's run to 1e-9, Agent.logs field for field, the rng in
    the reference's state."""
    d, meta, agg = capture(name)
    rng, auction = _auction(meta, tmp_path, meta["max_slots"])
    R = meta["rounds"]
    if how == "batch":
        auction.simulate_batch(R)
    else:
        for _ in range(R):
            auction.simulate_opportunity()
    rt = dict(rtol=1e-9, atol=1e-9)
    ag = auction.agents
    np.testing.assert_allclose([a.net_utility for a in ag], agg["net_utility"], **rt)
    np.testing.assert_allclose([a.gross_utility for a in ag], agg["gross_utility"], **rt)
    np.testing.assert_allclose([a.get_allocation_regret() for a in ag], agg["allocation_regret"], **rt)
    np.testing.assert_allclose([a.get_estimation_regret() for a in ag], agg["estimation_regret"], **rt)
    np.testing.assert_allclose([a.get_overbid_regret() for a in ag], agg["overbid_regret"], **rt)
    np.testing.assert_allclose([a.get_underbid_regret() for a in ag], agg["underbid_regret"], **rt)
    np.testing.assert_allclose(auction.revenue, agg["revenue"], **rt)
    st, after = rng.bit_generator.state, agg["rng_state_after"]
    assert (str(st["state"]["state"]), str(st["state"]["inc"]), st["has_uint32"], st["uinteger"]) == \
        (after["state"], after["inc"], after["has_uint32"], after["uinteger"])
    for a, agent in enumerate(ag):
        logs = agent.logs
        r, s = np.nonzero(d["part"] == a)
        assert len(logs) == len(r) == agg["n_logs"][a]
        for lg, rr, ss in zip(logs, r, s):
            assert (lg.item, lg.value, lg.bid) == (d["item"][rr, ss], d["slot_value"][rr, ss], d["slot_bid"][rr, ss])
            assert (lg.estimated_CTR, lg.true_CTR) == (d["slot_est_ctr"][rr, ss], d["slot_true_ctr"][rr, ss])
            assert lg.best_expected_value == d["slot_best_ev"][rr, ss]
            assert (lg.price, lg.second_price) == (d["slot_price"][rr, ss], d["slot_second_price"][rr, ss])
            assert (bool(lg.outcome), bool(lg.won)) == (bool(d["outcome"][rr, ss]), bool(d["won"][rr, ss]))
            assert np.array_equal(lg.context, np.append(d["ctx"][rr], 1.0))


def test_auction_refuses_learners_on_several_slots(gpu, tmp_path):
    _, meta, _ = capture("slots_fp_empirical_p3_s3")
    with pytest.raises(NotImplementedError, match="log-fed updates from multi-slot rounds"):
        _auction(meta, tmp_path, 3)
    _, meta, _ = capture("slots_sp_ts_p3_s3")
    with pytest.raises(NotImplementedError, match="log-fed updates from multi-slot rounds"):
        _auction(meta, tmp_path, 3)
    _, auction = _auction(meta, tmp_path, 1)  # one slot: as before
    assert auction.max_slots == 1
    _, meta, _ = capture("slots_fp_oracle_p4_s3")
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="positive integer"):
            _auction(meta, tmp_path, bad)
    with pytest.raises(NotImplementedError, match="at most 8"):
        _auction(meta, tmp_path, 9)
