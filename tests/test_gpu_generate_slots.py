"""Generate mode for multi-slot rounds on the GPU: ag_generate_slots, ag_simulate_slots_generated and
Auction(max_slots > 1).simulate_synthetic.

ag_generate_slots is held to the numpy statement tests/gen_slots_reference.py value for value (the
outputs are integers and doubles built from integers: exact). The fused call is held to the
three-call path -- ag_generate (+ ag_generate_noise) + ag_generate_slots, then ag_simulate_slots --
bit for bit in every ag_slots_out field and every counter limb, and, for OracleAllocator +
TruthfulBidder populations, to statements outside the project's device code: the oracle's
per-participant fields plus tests/slots_reference.py on the stated participants, slot counts and
uniforms (the contexts are the device generator's float32 Box-Muller normals, which
tests/gen_reference.py states only up to the hardware transcendentals' error; they are taken from
ag_generate, which tests/test_gpu_generator.py holds to that statement).
"""
import numpy as np
import pytest

import gen_reference as G
import gen_slots_reference as GS
import slots_records_reference as RR
import slots_reference as SR
from slots_cases import capture
from test_gpu_collect import _lrts_rows, _lrts_store_rows, _records
from test_gpu_slots import _auction as _oracle_auction
from test_gpu_slots import _catalogue, _compare
from test_gpu_slots_learners import _auction, _update_capture, engine_of, mixed

pytestmark = pytest.mark.gpu

SEEDS = (0, 0x9E3779B97F4A7C15)
CARRY = 2 ** 32 - 150  # the batch crosses the index's low word
FIRSTS = (0, CARRY, 5 * 10 ** 9)
BIG = (1 << 20) + 37  # one auction per lane, at most 2048 workgroups x 256 lanes = 2^19: three passes, a ragged last


# ---------------------------------------------------------------- helpers
def _tiny_engine(S, N=4, P=2, K=3, E=2):
    from auctiongym_amd.engine import AuctionEngine
    return AuctionEngine(N, P, K, E, min(E, 4), 0, 1.0, max_slots=S)


def _generate_slots(eng, seed, first, B, ns=True, us=True):
    """ag_generate_slots into poisoned arrays -> (num_slots [B], u_slots [S][B]) on the host."""
    import torch
    inp = {}
    if ns:
        inp["num_slots"] = torch.full((B,), -77, dtype=torch.int32, device=eng.device)
    if us:
        inp["u_slots"] = torch.full((eng.max_slots, B), -7.5, dtype=torch.float64, device=eng.device)
    eng.generate_slots(seed, first, inp)
    torch.cuda.synchronize()
    return tuple(inp[k].cpu().numpy() if k in inp else None for k in ("num_slots", "u_slots"))


def _oracle_engine(N, P, K, E, mech, S, seed):
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(seed)
    items, values = _catalogue(g, N, K, E)
    eng = AuctionEngine(N, P, K, E, min(E, 4), mech, 1.0, max_slots=S)
    eng.load_catalog(items, values)
    return eng, items, values


def mixed_no_search(seed, P, S, mech, N=10):
    """The shipped-shape mixed population of tests/test_gpu_slots.py with its ValueLearning bidder
    (agent 4) bidding from a fitted policy instead of by search: LR-TS sampling allocators beside
    Oracle ones; EmpiricalShaded, an uninitialised and fitted DoublyRobust, a fitted PolicyLearning."""
    from auctiongym_amd import _lib
    pop, _ = mixed(seed, P, S, mech, 1, N=N)
    pop["init"] = np.where(pop["init"] == _lib.LEARNER_SEARCH, _lib.LEARNER_POLICY, pop["init"]).astype(np.int32)
    pop["modes"] = np.full(N, _lib.VL_POLICY, np.int32)
    return pop


def _poisoned(eng, B, fields=None):
    out = eng.alloc_slot_outputs(B, fields)
    for v in out.values():  # poison: what a kernel must write is visible, the same for both paths
        v.fill_(77) if not v.dtype.is_floating_point else v.fill_(-7.5)
    return out


def three_call(eng, seed, first, B, counters=None, fields=None):
    """ag_generate (+ ag_generate_noise) + ag_generate_slots, then ag_simulate_slots."""
    inp = eng.alloc_inputs(B)
    eng.generate(seed, first, inp)
    if any(k in inp for k in ("gamma_raw", "ts_noise", "policy_eps")):
        eng.generate_noise(seed, first, inp)
    eng.generate_slots(seed, first, inp)
    out = _poisoned(eng, B, fields)
    eng.simulate_slots(inp, inp["num_slots"], inp["u_slots"], out, counters)
    return inp, out


def fused(eng, seed, first, B, counters=None, fields=None):
    out = _poisoned(eng, B, fields)
    eng.simulate_slots_generated(seed, first, out, counters)
    return out


def _bits(t):
    return t.cpu().numpy().tobytes()


def assert_same(got, want, what):
    """Every array bit for bit (NaNs included)."""
    assert set(got) == set(want), what
    for k in want:
        assert _bits(got[k]) == _bits(want[k]), (what, k)


def check_fused(eng, seed, first, B, what):
    """The fused call against the three-call path: every output field, every counter limb."""
    import torch
    c3, cf = eng.new_counters(), eng.new_counters()
    inp, want = three_call(eng, seed, first, B, c3)
    got = fused(eng, seed, first, B, cf)
    torch.cuda.synchronize()
    assert_same(got, want, what)
    assert _bits(cf) == _bits(c3), (what, "counters")
    assert int(c3.abs().sum().item()) > 0, what
    return inp, got, cf


def _rows(out):
    """Device ag_slots_out arrays -> row-major host arrays ([B][P], [B][S], [B])."""
    return {k: (np.ascontiguousarray(v.cpu().numpy().T) if v.dim() == 2 else v.cpu().numpy()) for k, v in out.items()}


# ---------------------------------------------------------------- 1. ag_generate_slots
@pytest.mark.parametrize("S", [1, 2, 3, 8])
def test_generate_slots_is_the_statement(gpu, S):
    """Every value of num_slots and u_slots, exact: both seeds, first index 0, at the index carry
    and 5e9, B around a wave and four workgroups with a ragged tail; either output NULL."""
    eng = _tiny_engine(S)
    for seed in SEEDS:
        for first in FIRSTS:
            for B in (1, 63, 65, 1000):
                idx = G.indices(first, B)
                ns, us = _generate_slots(eng, seed, first, B)
                assert ns.dtype == np.int32 and np.array_equal(ns, GS.num_slots(seed, idx, S)), (seed, first, B)
                assert us.shape == (S, B) and np.array_equal(us, GS.u_slots(seed, idx, S)), (seed, first, B)
                assert S > 1 or (ns == 1).all()
            ns1, none = _generate_slots(eng, seed, first, 65, us=False)
            none2, us1 = _generate_slots(eng, seed, first, 65, ns=False)
            assert none is None and none2 is None
            assert np.array_equal(ns1, ns[:65]) and np.array_equal(us1, us[:, :65])
    # row 0 is ag_generate's u: the batch is the one-slot batch with the slot draws beside it
    inp = eng.alloc_inputs(1000)
    eng.generate(SEEDS[1], CARRY, inp)
    assert np.array_equal(inp["u"].cpu().numpy(), _generate_slots(eng, SEEDS[1], CARRY, 1000)[1][0])
    eng.close()


def test_generate_slots_second_grid_stride_pass(gpu):
    """B = 2^20 + 37: the grid-stride loop's second pass, and 37 auctions in a third."""
    S = 3
    eng = _tiny_engine(S)
    ns, us = _generate_slots(eng, SEEDS[1], CARRY, BIG)
    eng.close()
    idx = G.indices(CARRY, BIG)
    assert np.array_equal(ns, GS.num_slots(SEEDS[1], idx, S))
    assert np.array_equal(us, GS.u_slots(SEEDS[1], idx, S))
    assert len(np.unique(ns[1 << 20:])) == S  # the last pass drew every count


@pytest.mark.parametrize("first", FIRSTS)
def test_generate_slots_three_launches_equal_one(gpu, first):
    eng = _tiny_engine(8)
    B, cuts = 1000, (0, 300, 301, 1000)
    ns, us = _generate_slots(eng, 7, first, B)
    parts = [_generate_slots(eng, 7, first + lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])]
    eng.close()
    assert np.array_equal(np.concatenate([p[0] for p in parts]), ns)
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), us)


# ---------------------------------------------------------------- 2. the fused call: Oracle + Truthful populations
@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("P", [1, 2, 3, 9, 16])
def test_fused_oracle_populations(gpu, oracle, P, S):
    """Both mechanisms x D in {2, 6, 8}, B = 300 (two workgroups, a ragged tail): the fused call
    equals the three-call path, and both equal the oracle's per-participant fields plus
    tests/slots_reference.py on the stated participants, slot counts and uniforms. K, the seed, the
    first index and the item search (screened / exact) vary with the case."""
    B = 300
    for mech in (0, 1):
        for D in (2, 6, 8):
            n = P * 7 + S * 3 + mech + D
            K, E, N = (3, 7, 12, 16)[n % 4], D - 1, P + 3
            seed, first = SEEDS[n % 2], FIRSTS[n % 3]
            eng, items, values = _oracle_engine(N, P, K, E, mech, S, 9300 + n)
            if n % 5 == 0:
                eng.set_item_search(True)
            what = f"P={P} S={S} mech={mech} D={D} K={K} seed={seed:#x} first={first}"
            inp, got, cnt = check_fused(eng, seed, first, B, what)
            eng.close()
            # ... and the independent expectation
            idx = G.indices(first, B)
            part = np.ascontiguousarray(G.participants(seed, idx, N, P).T)
            ns, us = GS.num_slots(seed, idx, S), np.ascontiguousarray(GS.u_slots(seed, idx, S).T)
            assert np.array_equal(inp["part"].cpu().numpy().T, part), what
            ctx = np.ascontiguousarray(inp["ctx"].cpu().numpy().T)
            orc = oracle.simulate(mech, items, values, ctx, part, us[:, 0])
            exp = SR.simulate(mech, orc, part, ns, us, S, N=N)
            assert np.array_equal(exp["num_filled"], np.minimum(ns, P - 1)), what
            host = dict(_rows(got), counters_fx=cnt.cpu().numpy())
            _compare(host, orc, exp, what)


# ---------------------------------------------------------------- 3. the shipped-shape mixed population
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("S", [3, 8])
@pytest.mark.parametrize("P", [3, 9, 16])
def test_fused_mixed_population(gpu, P, S, mech):
    """LR-TS Thompson noise, shading and rsample draws made in the kernel: at the index carry,
    B = 1000 and B = 1."""
    pop = mixed_no_search(9400 + 4 * P + S + mech, P, S, mech, N=max(10, P + 2))
    eng = engine_of(pop)
    for B in (1000, 1):
        _, got, _ = check_fused(eng, SEEDS[1], CARRY, B, f"mixed P={P} S={S} mech={mech} B={B}")
    o = _rows(fused(eng, SEEDS[1], CARRY, 1000))
    eng.close()
    assert np.isfinite(o["gamma"]).any() and np.isfinite(o["propensity"]).any()
    assert (o["num_filled"] == min(S, P - 1)).any() and (o["num_filled"] == 1).any()


@pytest.mark.parametrize("pop", ["oracle", "mixed"])
def test_fused_split_launches_null_counters_and_null_outputs(gpu, pop):
    """[first, first + B) in three launches with accumulated counters equals one launch (the draws
    depend on the global index alone); counters_fx NULL and the per-slot outputs NULL change
    nothing else."""
    import torch
    B, cuts, first, seed, S = 1000, (0, 300, 301, 1000), CARRY - 400, 11, 3
    if pop == "oracle":
        eng, _, _ = _oracle_engine(8, 4, 7, 5, 1, S, 9500)
    else:
        eng = engine_of(mixed_no_search(9501, 3, S, 0))
    cnt = eng.new_counters()
    one = fused(eng, seed, first, B, cnt)
    acc = eng.new_counters()
    parts = [fused(eng, seed, first + lo, hi - lo, acc) for lo, hi in zip(cuts, cuts[1:])]
    eng.set_launch_auctions(400)  # ... and the library's own split of one call
    capped_cnt = eng.new_counters()
    capped = fused(eng, seed, first, B, capped_cnt)
    eng.set_launch_auctions(0)
    torch.cuda.synchronize()
    assert_same({k: torch.cat([p[k] for p in parts], dim=-1) for k in one}, one, "three launches")
    assert _bits(acc) == _bits(cnt) and _bits(capped_cnt) == _bits(cnt)
    assert_same(capped, one, "AG_OPT_LAUNCH_AUCTIONS")
    assert_same(fused(eng, seed, first, B, None), one, "counters_fx NULL")
    per_slot = ("winner", "price", "second_price", "outcome", "log_price", "num_filled", "won_slot")
    rest = [f for f in one if f not in per_slot]
    cnt2 = eng.new_counters()
    got = fused(eng, seed, first, B, cnt2, fields=rest)
    torch.cuda.synchronize()
    assert_same(got, {k: one[k] for k in rest}, "per-slot outputs NULL")
    assert _bits(cnt2) == _bits(cnt)
    cnt3 = eng.new_counters()
    eng.simulate_slots_generated(seed, first, {"num_filled": one["num_filled"].clone().fill_(0)}, cnt3)
    assert _bits(cnt3) == _bits(cnt)  # B from the one array there is
    eng.close()


# ---------------------------------------------------------------- 4. a one-slot context
@pytest.mark.parametrize("mech", [0, 1])
@pytest.mark.parametrize("pop", ["oracle", "mixed"])
def test_one_slot_context_equals_simulate_generated(gpu, pop, mech):
    """num_slots = 1: winner, price, second price, outcome and the counter limbs of
    ag_simulate_generated (k_oracle / the per-P generate-mode builds)."""
    import torch
    B, seed, first, P = 1000, SEEDS[1], CARRY, 3
    if pop == "oracle":
        eng, _, _ = _oracle_engine(8, P, 12, 5, mech, 1, 9600 + mech)
    else:
        eng = engine_of(mixed_no_search(9610 + mech, P, 1, mech))
    cs, c1 = eng.new_counters(), eng.new_counters()
    got = fused(eng, seed, first, B, cs)
    out = eng.alloc_outputs(B)
    eng.simulate_generated(seed, first, out, c1)
    torch.cuda.synchronize()
    eng.close()
    for k in ("winner", "price", "second_price", "outcome"):
        assert _bits(got[k][0]) == _bits(out[k]), k
    for k in ("item", "bid", "est_ctr", "true_ctr", "best_ev") + (("gamma", "propensity") if pop == "mixed" else ()):
        assert _bits(got[k]) == _bits(out[k]), k
    assert (got["num_filled"] == 1).all() and _bits(got["log_price"]) == _bits(out["price"])
    assert _bits(cs) == _bits(c1)


# ---------------------------------------------------------------- 5. refusals
def test_refusals(gpu):
    import ctypes
    from auctiongym_amd import _lib
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(9700)
    # P = 17: the three-call path serves it, the fused call names its limit
    eng, _, _ = _oracle_engine(20, 17, 7, 5, 0, 3, 9700)
    with pytest.raises(NotImplementedError, match=r"ag_simulate_slots_generated: P <= 16 \(P=17\)"):
        fused(eng, 0, 0, 8)
    inp, out = three_call(eng, 0, 0, 8)
    assert int(out["num_filled"].min().item()) >= 1
    eng.close()
    # a ValueLearningBidder bidding by search
    pop, _ = mixed(9701, 3, 3, 0, 1)
    eng = engine_of(pop)
    with pytest.raises(NotImplementedError, match="ag_simulate_slots_generated: ValueLearningBidders bidding by search"):
        fused(eng, 0, 0, 8)
    eng.close()
    # a general population outside the shipped shape (OE = 3)
    N, K, E, OE = 6, 12, 5, 3
    items, values = _catalogue(g, N, K, E)
    eng = AuctionEngine(N, 3, K, E, OE, 0, 1.0, max_slots=3)
    eng.set_agent_params(np.array([1, 0, 1, 0, 1, 0], np.int32), np.zeros(N, np.int32))
    eng.load_catalog(items, values)
    eng.load_lrts(g.normal(0, 1, (N, K, OE + 1)).astype(np.float32), np.ones((N, K, OE + 1), np.float32))
    with pytest.raises(NotImplementedError, match=r"general populations in the shipped shape only \(E = 5, OE = 4; E=5 OE=3\)"):
        fused(eng, 0, 0, 8)
    # a NULL out
    rc = eng.L.ag_simulate_slots_generated(eng._h, 0, 0, 8, None, None, None)
    assert rc == _lib.AG_ERR_INVALID and b"ag_simulate_slots_generated: null argument" in eng.L.ag_last_error()
    rc = eng.L.ag_generate_slots(None, 0, 0, 8, None, None, None)
    assert rc == _lib.AG_ERR_INVALID
    so = _lib.AgSlotsOut()
    so.struct_size = 8  # not an ag_slots_out
    assert eng.L.ag_simulate_slots_generated(eng._h, 0, 0, 8, ctypes.byref(so), None, None) == _lib.AG_ERR_INVALID
    eng.close()


# ---------------------------------------------------------------- 6. Auction(max_slots = 3).simulate_synthetic
def _fx(limbs):
    return int(limbs[0]) + (int(limbs[1]) << 42) + (int(limbs[2]) << 84)


def _check_account(auction, cnt):
    """The agents' exact sums and the revenue against an engine-level run's counter limbs."""
    from auctiongym_amd import _lib
    limbs = cnt.cpu().numpy()
    paid = 0
    for a, agent in enumerate(auction.agents):
        for c in range(_lib.NUM_COUNTERS):
            assert agent._fx[c] == _fx(limbs[a, c]), (a, c)
        paid += _fx(limbs[a, _lib.COUNTERS.index("paid")])
    assert auction._revenue_fx == paid > 0


def test_auction_simulate_synthetic(gpu, tmp_path):
    """An Oracle population's fixture config at max_slots = 3: the agents' counters and the revenue
    are the engine-level three-call run's, the logs are kept, and a second call continues at
    first_auction."""
    import torch
    _, meta, _ = capture("slots_fp_oracle_p4_s3")
    _, auction = _oracle_auction(meta, tmp_path, meta["max_slots"])
    assert auction.max_slots == 3
    B, seed = 1000, 5
    auction.simulate_synthetic(B, seed)
    auction.simulate_synthetic(300, seed, first_auction=B)
    eng = auction._engine
    cnt = eng.new_counters()
    three_call(eng, seed, 0, B, cnt)
    _, out = three_call(eng, seed, B, 300, cnt)
    torch.cuda.synchronize()
    _check_account(auction, cnt)
    assert sum(a.num_logs() for a in auction.agents) == (B + 300) * meta["P"]
    assert _bits(auction._log_batches[-1][1]["won_slot"]) == _bits(out["won_slot"])


@pytest.mark.parametrize("name", ["slots_update_sp_ts", "slots_update_fp_empirical"])
def test_auction_simulate_synthetic_feeds_the_learners(gpu, tmp_path, name):
    """learners_on_slots=True: the records collected from a synthetic batch are
    tests/slots_records_reference.py's on the generated inputs and the device's outputs, LR-TS
    samples and shading records; Agent.update then trains on them."""
    import torch
    _, meta = _update_capture(name)
    torch.manual_seed(meta.get("torch_seed", 0))
    _, auction, _, _ = _auction(meta, tmp_path, learners_on_slots=True)
    assert auction.max_slots == 3 and auction._ts_agent[auction._lrts].all()
    B, seed, P = 1000, SEEDS[1], meta["P"]
    auction.simulate_synthetic(B, seed)
    eng = auction._engine
    cnt = eng.new_counters()
    inp, out = three_call(eng, seed, 0, B, cnt)
    torch.cuda.synchronize()
    _check_account(auction, cnt)
    o = _rows(out)
    if not eng.shading:
        o["gamma"] = o["propensity"] = np.full((B, P), np.nan)
    idx = G.indices(0, B)
    part = np.ascontiguousarray(G.participants(seed, idx, meta["N"], P).T)
    assert np.array_equal(inp["part"].cpu().numpy().T, part)
    assert np.array_equal(inp["num_slots"].cpu().numpy(), GS.num_slots(seed, idx, 3))
    ctx = np.ascontiguousarray(inp["ctx"].cpu().numpy().T)
    ak, bk = auction._lrts.astype(np.int32), auction._empirical.astype(np.int32)
    want = RR.expected_records_slots(part, o, bk, auction._values, P, 0)
    key, x = RR.expected_lrts_samples_slots(ctx, part, o, ak, meta["OE"], P)
    if name == "slots_update_sp_ts":
        st = auction._stores["lrts"]
        assert int(st["count"].item()) == len(key) > B and "shading" not in auction._stores
        assert np.array_equal(_lrts_store_rows(st), _lrts_rows(key, x))
    else:
        st = auction._stores["shading"]
        assert len(want["order"]) == B * P and "lrts" not in auction._stores and len(key) == 0
        got = _records(st)  # an EmpiricalShaded store keeps (agent, gamma, utility): no order, a multiset
        assert set(got) == {"agent", "gamma", "utility"} and len(got["agent"]) == B * P

        def rows(r):
            m = np.stack([np.asarray(r["agent"], np.int64).view(np.uint64), np.asarray(r["gamma"], np.float64).view(np.uint64),
                          np.asarray(r["utility"], np.float64).view(np.uint64)], axis=1)
            return m[np.lexsort(m.T[::-1])]
        assert np.array_equal(rows(got), rows(want)), name
        assert (want["utility"] != 0).any() and want["won"].any()
    before = [getattr(a.bidder, "prev_gamma", None) for a in auction.agents]
    for a in auction.agents:
        a.update(iteration=0)
    if name == "slots_update_sp_ts":
        assert all(a.allocator.epochs > 0 for a in auction.agents)
    else:
        assert all(a.bidder.prev_gamma != g0 for a, g0 in zip(auction.agents, before))
