"""The exact counters at the edges of their fixed-point range (needs an MI355X; `-m gpu`).

The ladder of tests/test_counter_reference.py -- values up to 2^26 and beyond, ties of the
rounding, negative totals, CTRs of exactly 0 and 1 and denormal ones -- through every kernel path
that accumulates counters. Every case compares all output fields and all 36 * N limbs with the
oracle (test_00_configs_gpu._compare) and the limbs with the plain statement of the counters
(tests/counter_reference.py, computed from the oracle's outputs). Inputs are made on the host with
fixed seeds and uploaded as in tests/test_gpu_shapes.py; the oracle's answer and the statement of
a case are computed once and shared. Nothing here has a tolerance: every comparison is on integers.

  * k_simulate<kGenOracle>, screened and exact scan: every rung, N = P in {2, 4}, both mechanisms;
  * k_oracle (default options): the rungs whose values it admits;
  * the loop rung: one workgroup per CU looping over >= 4 tiles (about 2.6e5 auctions);
  * the two-auctions-per-lane option (no such build ships: the one-auction kernel it falls back
    to), the runtime-P kernel (P = 9), 1024-lane workgroups: mid / high;
  * LR-TS + truthful (kGenTruthful) and the full mix at N = P = 8 (kGenAll) on mid, high,
    negative and zero-ctr: ALLOC_REGRET, EST_REGRET, CTR_SQERR and CTR_BIAS;
  * generate mode: k_oracle on boundary-lo and zero-ctr, the general kernel on a high catalogue
    in the shipped shape; an Oracle population it does not take is refused;
  * accumulation into a preloaded buffer: a carry into limb 2, a total crossing zero, limbs as an
    8-rank all-reduce leaves them, three calls with odd split points, six launches per call.
"""
import numpy as np
import pytest

import counter_reference as R
from test_00_configs_gpu import _compare
from test_counter_reference import (B_LADDER, E, K, RUNGS, SMALL_RUNGS, TWO26, _catalogue, check_rung, ladder_case,
                                    limbs)
from test_gpu_shapes import _ALL_FIELDS, _general_setup, _host, _oracle_engine, _simulate, _upload

pytestmark = pytest.mark.gpu

_cache = {}


def _case(oracle, name, N, mech, B=B_LADDER):
    """(case, the oracle's answer, the statement's limbs) of a rung -- computed once; the rung's
    condition is asserted on the way."""
    key = (name, N, mech, B)
    if key not in _cache:
        case = ladder_case(name, N, B)
        orc = oracle.simulate(mech, case["items"], case["values"], case["ctx"], case["part"], case["u"],
                              nthreads=16 if B > 4096 else 1)
        if B == B_LADDER:
            check_rung(case, orc)
        _cache[key] = (case, orc, limbs(R.counters(orc, case["part"], N, N)))
    return _cache[key]


def _check(out, cnt, orc, want, what):
    _compare(out, cnt, orc, what)
    assert np.array_equal(cnt.cpu().numpy(), want), (what, "the plain statement")


def _engine(case, mech):
    return _oracle_engine(case["N"], case["N"], K, E, mech, case["items"], case["values"])


def _inputs(eng, case):
    return _upload(eng, case["ctx"], case["part"], case["u"])


# ---------------------------------------------------------------- k_simulate<kGenOracle>, every rung
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("name", [r for r in RUNGS if r != "loop"])
def test_ladder_general_kernel(gpu, oracle, name, N):
    """k_simulate<P, 3, PRUNE, 1, kGenOracle> screened (AG_SIM_KERNEL_GENERIC) and with the exact scan,
    both mechanisms. boundary-hi also against boundary-lo through the same kernel: one value one
    ulp apart, so every auction in which that item is chosen by nobody has the same outputs."""
    for mech in (0, 1):
        case, orc, want = _case(oracle, name, N, mech)
        eng = _engine(case, mech)
        inp = _inputs(eng, case)
        eng.set_simulate_kernel(True)
        out, cnt = _simulate(eng, inp, B_LADDER)
        _check(out, cnt, orc, want, f"{name} N={N} mech={mech} screened")
        eng.set_item_search(True)
        _check(*_simulate(eng, inp, B_LADDER), orc, want, f"{name} N={N} mech={mech} exact")
        eng.close()
        if name == "boundary-hi":
            # default options: one value of exactly 1024.0 is outside k_oracle's (0, 1024), so the
            # dispatch itself falls back to k_simulate; one ulp less (boundary-lo) stays on k_oracle
            eng = _engine(case, mech)
            _check(*_simulate(eng, inp, B_LADDER), orc, want, f"{name} N={N} mech={mech} default options")
            with pytest.raises(NotImplementedError, match=r"ag_simulate_generated: .*catalogue values in \(0, 1024\)"):
                eng.simulate_generated(0, 0, eng.alloc_outputs(64))  # k_oracle-only there: the boundary, observed
            eng.close()
            lo_case, lo_orc, lo_want = _case(oracle, "boundary-lo", N, mech)
            assert all(np.array_equal(case[k], lo_case[k]) for k in ("items", "ctx", "part", "u"))
            eng = _engine(lo_case, mech)
            eng.set_simulate_kernel(True)
            lo_out, lo_cnt = _simulate(eng, _inputs(eng, lo_case), B_LADDER)
            _check(lo_out, lo_cnt, lo_orc, lo_want, f"boundary-lo N={N} mech={mech} screened")
            hi, lo = _host(out, cnt), _host(lo_out, lo_cnt)
            edge = (case["part"] == 0) & (hi["item"] == 1)  # agent 0's item 1 holds the edge value
            assert np.array_equal(edge, (case["part"] == 0) & (lo["item"] == 1))
            same = ~edge.any(axis=1)
            assert 50 <= same.sum() <= B_LADDER - 50
            for k in ("winner", "price", "second_price", "outcome", "item", "bid", "est_ctr", "true_ctr", "best_ev"):
                assert np.array_equal(hi[k][same], lo[k][same]), k
            eng.close()


@pytest.mark.parametrize("N,mech", [(2, 0), (4, 1)], ids=["N2_fp", "N4_sp"])
def test_loop_rung(gpu, oracle, N, mech):
    """Values just below 2^24 (terms of 2^59) with one workgroup per CU and B = 4 * 256 * CUs + 37:
    every workgroup loops over at least four tiles, so a replica cell takes >= 64 such terms. Two
    agents under FirstPrice, four under SecondPrice."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 4 * 256 * cus + 37
    case, orc, want = _case(oracle, "loop", N, mech, B)
    assert (orc["best_ev"] >= 2.0 ** 22).all()
    wins = np.bincount(case["part"][np.arange(B), orc["winner"]], minlength=N)
    assert (wins * 10 >= B).all()
    eng = _engine(case, mech)
    eng.set_blocks_per_cu(1)
    eng.set_simulate_kernel(True)
    inp = _inputs(eng, case)
    _check(*_simulate(eng, inp, B), orc, want, f"loop N={N} B={B} screened")
    eng.set_item_search(True)
    _check(*_simulate(eng, inp, B), orc, want, f"loop N={N} B={B} exact")
    eng.close()
    _cache.pop(("loop", N, mech, B))  # a quarter of a million auctions: not kept for the session


# ---------------------------------------------------------------- k_oracle
@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("name", SMALL_RUNGS)
def test_ladder_oracle_kernel(gpu, oracle, name, N):
    """k_oracle<P, 3> (default options) on the rungs whose values lie in (0, 1024), both mechanisms."""
    for mech in (0, 1):
        case, orc, want = _case(oracle, name, N, mech)
        assert ((case["values"] > 0) & (case["values"] < 1024)).all()
        eng = _engine(case, mech)
        _check(*_simulate(eng, _inputs(eng, case), B_LADDER), orc, want, f"k_oracle {name} N={N} mech={mech}")
        eng.close()


# ---------------------------------------------------------------- other builds of k_simulate
def _head(case, B):
    return dict(case, ctx=case["ctx"][:B], part=case["part"][:B], u=case["u"][:B])


@pytest.mark.parametrize("name", ["mid", "high"])
def test_two_auctions_per_lane(gpu, oracle, name):
    """AG_OPT_LANE_AUCTIONS = 2 on an even batch (the first 548 auctions of the rung). The shipped
    library builds no two-auctions-per-lane kernel: ag_simulate then takes the one-auction build
    of k_simulate, so here this pins the option's even-batch dispatch (and keeps an Oracle
    population with the option set off k_oracle)."""
    for N, mech in ((2, 1), (4, 0)):
        case = _head(ladder_case(name, N), 548)
        orc = oracle.simulate(mech, case["items"], case["values"], case["ctx"], case["part"], case["u"])
        assert (orc["best_ev"] >= (2.0 ** 13 if name == "mid" else 2.0 ** 24)).all()
        want = limbs(R.counters(orc, case["part"], N, N))
        eng = _engine(case, mech)
        eng.set_lane_auctions(2)
        _check(*_simulate(eng, _inputs(eng, case), 548), orc, want, f"two per lane {name} N={N}")
        eng.close()


def test_runtime_p_kernel_high(gpu, oracle):
    """k_simulate<0, 3, ...> (N = P = 9) on the high catalogue, screened and exact."""
    N = 9
    case = ladder_case("high", N, seed=4900)
    for mech in (0, 1):
        orc = oracle.simulate(mech, case["items"], case["values"], case["ctx"], case["part"], case["u"])
        assert (orc["best_ev"] >= 2.0 ** 24).all() and len(set(case["part"][np.arange(B_LADDER), orc["winner"]])) >= 5
        want = limbs(R.counters(orc, case["part"], N, N))
        eng = _engine(case, mech)
        inp = _inputs(eng, case)
        _check(*_simulate(eng, inp, B_LADDER), orc, want, f"runtime-P high mech={mech} screened")
        eng.set_item_search(True)
        _check(*_simulate(eng, inp, B_LADDER), orc, want, f"runtime-P high mech={mech} exact")
        eng.close()


def _population_case(oracle, name, pop, N, P, mech, seed, bt=0):
    """A general population (tests/test_gpu_shapes._population) on the rung's catalogue: engine,
    device outputs, the oracle's answer and the statement's table."""
    from auctiongym_amd import _lib
    items, values = _catalogue(name, N, np.random.default_rng(seed))
    eng, (ctx, part, u, more), orc, _ = _general_setup(seed + 1, N, P, K, E, E, mech, pop, catalogue=(items, values))
    if bt:
        eng._check(eng.L.ag_set_option(eng._h, _lib.OPT_SIM_BLOCK_THREADS, bt), "ag_set_option")
    out, cnt = _simulate(eng, _upload(eng, ctx, part, u, **more), B_LADDER, _ALL_FIELDS if pop == "all" else None)
    o = orc(oracle)
    table = R.counters(o, part, P, N)
    _check(out, cnt, o, limbs(table), f"{pop} {name} N={N} P={P} mech={mech} bt={bt}")
    eng.close()
    return o, table


_GENERAL_SLOTS = (R.ALLOC_REGRET, R.EST_REGRET, R.CTR_SQERR, R.CTR_BIAS)


@pytest.mark.parametrize("pop", ["ts", "all"])
@pytest.mark.parametrize("name", ["mid", "high", "negative", "zero-ctr"])
def test_ladder_general_populations(gpu, oracle, name, pop):
    """kGenTruthful (LR-TS + truthful, N = P = 4) and kGenAll (the full mix, N = P = 8: every bidder
    kind) -- the slots an Oracle population never fills. On zero-ctr the LR-TS agents' est / 0 terms
    are dropped and the mix's Oracle allocators count 1 per won record (the CTR-bias rule); they bid
    0 and win only against each other, so that case draws P = 2 of the 8."""
    N = 8 if pop == "all" else 4
    P = 2 if (pop, name) == ("all", "zero-ctr") else N
    mech = (RUNGS.index(name) + (pop == "all")) % 2
    o, table = _population_case(oracle, name, pop, N, P, mech, 5000 + 10 * RUNGS.index(name) + N)
    lrts = [a for a in range(N) if pop == "ts" or a % 2 == 1]
    if name == "zero-ctr":
        assert (o["true_ctr"] == 0).all()
        won = [table[a][R.N_WON] for a in range(N)]
        assert sum(won) == B_LADDER << 36
        for a in range(N):
            if a in lrts:  # est / 0: dropped
                assert table[a][R.CTR_BIAS] == 0 and won[a] > 0, a
            else:          # 0 / 0 between equal bits: 1 per won record
                assert table[a][R.CTR_BIAS] == won[a] > 0, a
    else:
        for a in lrts:  # CTR_BIAS is summed over won records only
            assert all(table[a][c] != 0 for c in _GENERAL_SLOTS[:3]), (a, table[a])
            assert (table[a][R.CTR_BIAS] != 0) == (table[a][R.N_WON] != 0), (a, table[a])
        assert any(table[a][R.CTR_BIAS] != 0 for a in lrts)
        big = 2.0 ** (13 if name == "mid" else 24 if name == "high" else 0)
        assert (np.abs(o["best_ev"]) >= big).all()
        if name == "negative":
            assert min(min(row) for row in table) < 0


def test_1024_lane_workgroups_high(gpu, oracle):
    """AG_OPT_SIM_BLOCK_THREADS = 1024 (the general kernel's large-image build) on the high catalogue."""
    o, _ = _population_case(oracle, "high", "all", 8, 8, 0, 5300, bt=1024)
    assert (o["best_ev"] >= 2.0 ** 24).all()


# ---------------------------------------------------------------- generate mode
def _replay_generated(eng, B, seed, first, noise=False):
    """ag_generate (+ ag_generate_noise) + ag_simulate against ag_simulate_generated: every output
    and limb equal. Returns the replay's device outputs, limbs and inputs."""
    import torch
    inp = eng.alloc_inputs(B)
    eng.generate(seed, first, inp)
    if noise:
        eng.generate_noise(seed, first, inp)
    out, cnt = eng.alloc_outputs(B), eng.new_counters()
    eng.simulate(inp, out, cnt)
    out_g, cnt_g = eng.alloc_outputs(B), eng.new_counters()
    eng.simulate_generated(seed, first, out_g, cnt_g)
    torch.cuda.synchronize()
    for k in out:
        assert np.array_equal(out[k].cpu().numpy(), out_g[k].cpu().numpy(), equal_nan=True), k
    assert torch.equal(cnt, cnt_g)
    return out, cnt, inp


@pytest.mark.parametrize("name", ["boundary-lo", "zero-ctr"])
def test_generate_mode_oracle_kernel(gpu, oracle, name):
    """k_oracle drawing its own inputs: equal to the replay of ag_generate's, which equals the oracle
    and the statement on the downloaded inputs."""
    N, mech, first = 2, 1, 123456789012
    case = ladder_case(name, N)
    eng = _engine(case, mech)
    out, cnt, inp = _replay_generated(eng, B_LADDER, 42, first)
    ctx, part, u = inp["ctx"].cpu().numpy().T, inp["part"].cpu().numpy().T, inp["u"].cpu().numpy()
    orc = oracle.simulate(mech, case["items"], case["values"], ctx, part, u)
    if name == "zero-ctr":
        assert (orc["true_ctr"] == 0).all()
    _check(out, cnt, orc, limbs(R.counters(orc, part, N, N)), f"generate {name}")
    eng.close()


def test_generate_mode_high_values(gpu, oracle):
    """Generate mode on a high catalogue. An Oracle population outside k_oracle's bounds is refused;
    the general kernel draws its inputs in the shipped shape only (E = 5, OE = 4), so the terms of
    2^62 go through it there: LR-TS + truthful, K = 3, N = P = 2."""
    from auctiongym_amd.engine import AuctionEngine
    case = ladder_case("high", 2)
    eng = _engine(case, 1)
    with pytest.raises(NotImplementedError, match=r"ag_simulate_generated: .*catalogue values in \(0, 1024\)"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(64))
    eng.close()
    N, E5, OE, mech, first = 2, 5, 4, 0, 98765432109
    g = np.random.default_rng(5400)
    items = np.concatenate([g.normal(0, 0.1, (N, K, E5)), 3.49 + 0.02 * g.random((N, K, 1))], axis=2)
    values = 0.99 * TWO26 * (1.0 - 2e-4 * g.random((N, K)))
    m = g.normal(0, 1, (N, K, OE + 1)).astype(np.float32)
    q = (0.5 + 3.0 * g.random((N, K, OE + 1))).astype(np.float32)
    ak, bk = np.ones(N, np.int32), np.zeros(N, np.int32)
    eng = AuctionEngine(N, N, K, E5, OE, mech, 1.0)
    eng.set_agent_params(ak, bk)
    eng.load_catalog(items, values)
    eng.load_lrts(m, q, thompson_sampling=True)
    out, cnt, inp = _replay_generated(eng, B_LADDER, 11, first, noise=True)
    ctx, part, u = inp["ctx"].cpu().numpy().T, inp["part"].cpu().numpy().T, inp["u"].cpu().numpy()
    noise = eng.untile_ts_noise(inp["ts_noise"], B_LADDER).reshape(B_LADDER, N, K, OE + 1)
    orc = oracle.simulate_pop(mech, items, values, ctx, part, u, ak, bk, OE=OE, ts_m=m, ts_noise=noise, ts_sample=True)
    assert (orc["best_ev"] >= 2.0 ** 24).all()
    _check(out, cnt, orc, limbs(R.counters(orc, part, N, N)), "generate high, shipped shape")
    eng.close()


# ---------------------------------------------------------------- accumulation
def _preloads(N):
    full = (1 << 42) - 1
    g = np.random.default_rng(77)
    carry = np.zeros((N, 12, 3), np.int64)
    carry[..., :2] = full
    minus_one = np.empty((N, 12, 3), np.int64)
    minus_one[...] = R.to_limbs(-1)
    ranks = np.concatenate([g.integers(0, 8 * full + 1, (N, 12, 2)), g.integers(-2 ** 40, 2 ** 40 + 1, (N, 12, 1))], axis=2)
    # the header's bound for a buffer that is not in normal form: |limb 0|, |limb 1| < 2^62, either sign
    edge = np.concatenate([g.integers(2 ** 62 - 2 ** 40, 2 ** 62, (N, 12, 2)) * g.choice([-1, 1], (N, 12, 2)),
                           g.integers(-2 ** 40, 2 ** 40 + 1, (N, 12, 1))], axis=2)
    edge[0, :, :2] = 2 ** 62 - 1
    edge[1, :, :2] = -(2 ** 62 - 1)
    return {"zero": np.zeros((N, 12, 3), np.int64), "carry": carry, "minus-one": minus_one, "all-reduced": ranks,
            "at-the-bound": edge}


@pytest.mark.parametrize("kernel", ["k_oracle", "k_simulate"])
def test_accumulation_into_preloaded_limbs(gpu, oracle, kernel):
    """The mid rung (N = P = 2; for k_oracle a copy with every value scaled by 2^-8) accumulated
    into a buffer that already holds limbs: all of limbs 0 and 1 at 2^42 - 1 (a carry ripples into
    limb 2), the value -1 in normal form (the total crosses zero), limbs as an 8-rank all-reduce
    leaves them (not normalised: the value is kept, limbs 0 and 1 come back normalised), limbs 0 and
    1 of either sign just inside the header's bound of 2^62 -- in one
    call, in three calls split at odd auctions, and as six launches per call. Always the limbs of
    to_limbs(from_limbs(preload) + statement)."""
    import torch
    N, mech, B = 2, 1, B_LADDER
    case = dict(ladder_case("mid", N))
    if kernel == "k_oracle":
        case["values"] = case["values"] * 2.0 ** -8
        assert (case["values"] < 1024).all()
    orc = oracle.simulate(mech, case["items"], case["values"], case["ctx"], case["part"], case["u"])
    table = R.counters(orc, case["part"], N, N)
    assert np.array_equal(orc["counters_fx"], limbs(table))
    eng = _engine(case, mech)
    eng.set_simulate_kernel(kernel == "k_simulate")
    inp = _inputs(eng, case)
    cuts = {"one call": (0, B), "three calls": (0, 131, 366, B)}
    for pname, pre in _preloads(N).items():
        want = np.array([[R.to_limbs(R.from_limbs(pre[a, c]) + table[a][c]) for c in range(12)] for a in range(N)],
                        dtype=np.int64)
        if pname == "carry":
            assert (want[:, R.N_LOGS, 2] == 1).all()
        if pname == "minus-one":
            assert (want[:, R.N_LOGS, 2] == 0).all() and (pre[..., 2] == -1).all()
        for mode in ("one call", "three calls", "six launches"):
            eng.set_launch_auctions(100 if mode == "six launches" else 0)
            cnt = torch.from_numpy(pre.copy()).to(eng.device)
            edges = cuts.get(mode, (0, B))
            for a, b in zip(edges[:-1], edges[1:]):
                part_inp = {k: (v[a:b] if v.dim() == 1 else v[:, a:b]).contiguous() for k, v in inp.items()}
                eng.simulate(part_inp, eng.alloc_outputs(b - a), cnt)
            torch.cuda.synchronize()
            got = cnt.cpu().numpy()
            assert np.array_equal(got, want), (kernel, pname, mode, np.argwhere(got != want)[:4].tolist())
    eng.close()
