"""The plain statement of the counters (tests/counter_reference.py) against the oracle, and the
ladder of catalogues that takes the exact counters to the edges of their fixed-point range.

The rest of the suite feeds the counters values near 1 and CTRs near 0.03. The ladder below is
shared with tests/test_gpu_counters.py: N = P (every agent in every auction), K = 3, E = 2,
embedding coefficients N(0, 0.1), B = 549. Each rung is built so that every agent wins at least a
tenth of the auctions -- the agents' best items are worth the same to within what the context moves
a CTR by -- and states the condition it is there for, which is asserted on the oracle's outputs.

  boundary-lo   values just below 1024, one equal to nextafter(1024, 0): the largest k_oracle admits
  boundary-hi   the same with that value = 1024.0: the fall-back to k_simulate
  ties-unit     (k + 1/2) * 2^-36 for even and odd k, near 1: round-half-even, fast branch
  ties-tiny1    every value 2^-37 (rounds to 0);  ties-tiny3: every value 3 * 2^-37 (rounds to 2)
  ties-big      2^14 - 2^-37 and 2^14: the same tie on both sides of the |x| < 2^14 branch
  mid           just below 2^17: the branch for |x| >= 2^14, sums inside the documented count
  high          just below 0.99 * 2^26: sixteen best-EV terms pass 2^63
  loop          just below 2^24: terms of 2^59, for a workgroup that loops over many tiles
  drop          around 2^26: GROSS terms at or above 2^26 dropped, PAID and BEST_EV kept
  negative      about -2: negative totals (limb 2 = -1);  mixed: items of both signs, exact scan
  zero-ctr      intercepts in (-800, -799): true CTR exactly 0, all bids 0, ties to slot 0
  one-ctr       intercepts in (40, 41): CTR exactly 1, every outcome 1, equal top values
  denormal-ctr  intercepts about -709.2 (and down to -745): denormal CTRs and bids

Intercepts are in (3, 4) unless the rung says otherwise; within it they are kept to (3.49, 3.51)
so that no agent's CTR decides every auction.
"""
from fractions import Fraction

import numpy as np
import pytest

import counter_reference as R
from conftest import load_capture, mech_code, pop_args

K, E, B_LADDER = 3, 2, 549
TWO26 = 2.0 ** 26


def _items(g, N, lo, hi):
    """[N][K][E + 1]: N(0, 0.1) coefficients and an intercept in (lo, hi)."""
    return np.concatenate([g.normal(0, 0.1, (N, K, E)), lo + (hi - lo) * g.random((N, K, 1))], axis=2)


def _cluster(g, N, top, spread=2e-4):
    """[N][K] values in (top * (1 - spread), top]."""
    return top * (1.0 - spread * g.random((N, K)))


def _tie_values(N, listed):
    """The listed values dealt round-robin over the N * K items."""
    return np.array([listed[i % len(listed)] for i in range(N * K)]).reshape(N, K)


TIES_UNIT = [(2.0 ** 36 + k + 0.5) * 2.0 ** -36 for k in (0, 1, 2, 3, 6, 9)]
TIES_BIG = [2.0 ** 14 - 2.0 ** -37, 2.0 ** 14]
EDGE_LO = float(np.nextafter(1024.0, 0.0))


def _catalogue(name, N, g):
    items = _items(g, N, 3.49, 3.51)
    if name in ("boundary-lo", "boundary-hi"):
        values = _cluster(g, N, EDGE_LO * (1 - 1e-6))
        values[0, 1] = EDGE_LO if name == "boundary-lo" else 1024.0
        items[0, 1, E] = 3.51  # the edge item is its agent's best at most contexts
    elif name == "ties-unit":
        values = _tie_values(N, TIES_UNIT)
    elif name == "ties-tiny1":
        values = np.full((N, K), 2.0 ** -37)
    elif name == "ties-tiny3":
        values = np.full((N, K), 3 * 2.0 ** -37)
    elif name == "ties-big":
        values = _tie_values(N, TIES_BIG)
    elif name == "mid":
        values = _cluster(g, N, 2.0 ** 17 * (1 - 1e-6))
    elif name == "high":
        values = _cluster(g, N, 0.99 * TWO26)
    elif name == "loop":
        values = _cluster(g, N, 2.0 ** 24 * (1 - 1e-6))
    elif name == "drop":
        values = TWO26 * (1.0 + 4e-4 * (g.random((N, K)) - 0.5))
        values[:, 0] = TWO26 * (1.0 + 1e-4 * np.where(np.arange(N) % 2 == 0, 1, -1))
    elif name == "negative":
        values = -_cluster(g, N, 2.0)
    elif name == "mixed":
        values = _cluster(g, N, 1.5)
        values[:, 1] = -2.0 - g.random(N)
    elif name == "zero-ctr":
        items, values = _items(g, N, -800.0, -799.0), 0.5 + g.random((N, K))
    elif name == "one-ctr":
        items, values = _items(g, N, 40.0, 41.0), np.tile([1.25, 1.0, 1.25], (N, 1))
    elif name == "denormal-ctr":
        items, values = _items(g, N, -709.25, -709.2), _cluster(g, N, 1.0)
        items[:, 2, E] = -745.0 + 25.0 * g.random(N)
    else:
        raise KeyError(name)
    return items, values


RUNGS = ("boundary-lo", "boundary-hi", "ties-unit", "ties-tiny1", "ties-tiny3", "ties-big", "mid", "high", "loop",
         "drop", "negative", "mixed", "zero-ctr", "one-ctr", "denormal-ctr")
# Fixed seeds: 4100 + 16 * (the rung's index) + N, plus the smallest multiple of 1000 under which the
# rung meets its condition in both mechanisms (an agent whose three items all drew small
# coefficients seldom has the best CTR; with four agents a few draws have one). check_rung asserts
# the conditions on every run, so a seed that stopped meeting them would fail, not pass quietly.
SEEDS = {("boundary-lo", 2): 4102, ("boundary-lo", 4): 6104, ("ties-unit", 2): 6134, ("ties-unit", 4): 4136,
         ("ties-tiny1", 2): 4150, ("ties-tiny1", 4): 7152, ("ties-tiny3", 2): 4166, ("ties-tiny3", 4): 7168,
         ("ties-big", 2): 4182, ("ties-big", 4): 6184, ("mid", 2): 4198, ("mid", 4): 10200, ("high", 2): 4214,
         ("high", 4): 8216, ("loop", 2): 4230, ("loop", 4): 8232, ("drop", 2): 4246, ("drop", 4): 6248,
         ("negative", 2): 4262, ("negative", 4): 8264, ("mixed", 2): 4278, ("mixed", 4): 5280,
         ("zero-ctr", 2): 4294, ("zero-ctr", 4): 4296, ("one-ctr", 2): 4310, ("one-ctr", 4): 4312,
         ("denormal-ctr", 2): 4326, ("denormal-ctr", 4): 9328}
# what k_oracle admits: every value in (0, 1024)
SMALL_RUNGS = ("boundary-lo", "ties-unit", "ties-tiny1", "ties-tiny3", "zero-ctr", "one-ctr", "denormal-ctr")


def ladder_case(name, N, B=B_LADDER, seed=None):
    """Catalogue and rounds of one rung: items [N][K][E + 1], values [N][K], ctx [B][E], part [B][N]
    (a random order of all N agents), u [B]. The boundary rungs share everything but one value."""
    if seed is None:
        seed = SEEDS["boundary-lo" if name == "boundary-hi" else name, N]
    g = np.random.default_rng(seed)
    items, values = _catalogue(name, N, g)
    ctx = g.normal(0, 1, (B, E))
    part = np.ascontiguousarray(np.argsort(g.random((B, N)), axis=1).astype(np.int32))
    return dict(name=name, N=N, items=items, values=values, ctx=ctx, part=part, u=g.random(B))


def chosen_value(o):
    """The value of the winner's item, per auction."""
    return o["value"][np.arange(len(o["winner"])), o["winner"]]


def check_rung(case, o):
    """The rung's stated condition, on the oracle's outputs o of the case (either mechanism)."""
    name, N, values = case["name"], case["N"], case["values"]
    wins = np.bincount(case["part"][np.arange(len(o["winner"])), o["winner"]], minlength=N)
    assert (wins * 10 >= len(o["winner"])).all(), (name, wins.tolist())  # every agent: >= 10 % of the auctions
    clicked = chosen_value(o)[o["outcome"] == 1]
    if name not in ("zero-ctr", "one-ctr", "denormal-ctr"):
        assert ((o["true_ctr"] > 0.9) & (o["true_ctr"] < 1)).all(), name
    if name == "boundary-lo":
        assert ((values > 0) & (values < 1024)).all() and (values == EDGE_LO).sum() == 1
        assert (clicked == EDGE_LO).any()
    elif name == "boundary-hi":
        assert (values > 0).all() and (values >= 1024).sum() == 1 and values.max() == 1024.0
        assert (clicked == 1024.0).any()
    elif name.startswith("ties"):
        listed = {"ties-unit": TIES_UNIT, "ties-tiny1": [2.0 ** -37], "ties-tiny3": [3 * 2.0 ** -37],
                  "ties-big": TIES_BIG}[name]
        for v in listed:  # at least one clicked win per listed value; its GROSS term is a tie
            assert (clicked == v).any(), (name, v)
            assert (Fraction(v) * 2 ** 36).denominator == 2 or v == 2.0 ** 14, (name, v)
    elif name == "mid":
        assert ((values >= 2.0 ** 14) & (values < 2.0 ** 17)).all() and (o["best_ev"] >= 2.0 ** 13).all()
    elif name == "high":
        assert ((values >= 0.6 * TWO26) & (values <= 0.99 * TWO26)).all() and (o["best_ev"] >= 2.0 ** 24).all()
    elif name == "loop":
        assert ((values >= 2.0 ** 23) & (values < 2.0 ** 24)).all() and (o["best_ev"] >= 2.0 ** 22).all()
    elif name == "drop":
        assert ((values >= 2.0 ** 25) & (values < 2.0 ** 27)).all()
        assert (clicked >= TWO26).sum() >= 50 and (clicked < TWO26).sum() >= 50, name  # dropped / kept GROSS terms
        assert (o["best_ev"] < TWO26).all() and (o["price"] < TWO26).all()            # PAID, BEST_EV: kept
    elif name == "negative":
        assert ((values > -3) & (values < -1)).all()
        assert min(min(row) for row in case_statement(case, o)) < 0
    elif name == "mixed":
        assert (values > 0).any() and (values < 0).any() and (chosen_value(o) > 0).all()
    elif name == "zero-ctr":
        assert (o["true_ctr"] == 0).all() and (o["bid"] == 0).all() and (o["winner"] == 0).all()
        assert (o["price"] == 0).all() and (wins > 0).all()
    elif name == "one-ctr":
        assert (o["true_ctr"] == 1.0).all() and (o["outcome"] == 1).all()
    elif name == "denormal-ctr":
        t = o["true_ctr"]
        assert ((t > 0) & (t < np.finfo(np.float64).tiny)).any() and (t < 1e-300).all()


def case_statement(case, o):
    return R.counters(o, case["part"], case["N"], case["N"])


def limbs(table):
    return np.array(R.limbs_of(table), dtype=np.int64)


# ---------------------------------------------------------------- the statement's own pieces
def test_fx_is_fraction_rounding():
    """fx(x) == round(Fraction(x) * 2**36) (ties to even) below 2^26, 0 from there on and for
    non-finite x: on ties in both directions, both signs, denormals and the edges of the range."""
    g = np.random.default_rng(1)
    xs = [0.0, -0.0, 2.0 ** -37, -2.0 ** -37, 3 * 2.0 ** -37, -3 * 2.0 ** -37, 5e-324, 2.0 ** 14, 2.0 ** 14 - 2.0 ** -37,
          float(np.nextafter(TWO26, 0)), -float(np.nextafter(TWO26, 0)), *TIES_UNIT, *TIES_BIG]
    xs += list(g.normal(0, 1, 200)) + list(g.normal(0, 1, 200) * 2.0 ** 25) + list((g.integers(-99, 99, 100) + 0.5) * 2.0 ** -36)
    for x in xs:
        want = round(Fraction(x) * 2 ** 36) if abs(x) < TWO26 else 0
        assert R.fx(x) == want, x
    assert [R.fx(x) for x in (2.0 ** -37, 3 * 2.0 ** -37, -2.0 ** -37, -3 * 2.0 ** -37)] == [0, 2, 0, -2]
    assert R.fx(2.0 ** 14 - 2.0 ** -37) == 2 ** 50 and R.fx(float(np.nextafter(TWO26, 0))) == 2 ** 62 - 2 ** 9
    for x in (TWO26, -TWO26, 2.0 ** 27, float("inf"), float("-inf"), float("nan"), 1e308):
        assert R.fx(x) == 0, x


def test_limbs_round_trip():
    """to_limbs gives the normal form (limbs 0, 1 in [0, 2^42), limb 2 signed); from_limbs inverts it
    and takes limbs in any form."""
    g = np.random.default_rng(2)
    vals = [0, 1, -1, 2 ** 42 - 1, 2 ** 42, -2 ** 42, 2 ** 84 - 1, 2 ** 84, -2 ** 84, -2 ** 84 - 1, 2 ** 100 + 12345]
    vals += [int(a) * int(b) for a, b in g.integers(-2 ** 62, 2 ** 62, (200, 2))]
    for v in vals:
        l0, l1, l2 = R.to_limbs(v)
        assert 0 <= l0 < 2 ** 42 and 0 <= l1 < 2 ** 42 and R.from_limbs([l0, l1, l2]) == v, v
    assert R.to_limbs(-1) == [2 ** 42 - 1, 2 ** 42 - 1, -1]
    assert R.from_limbs([8 * (2 ** 42 - 1), -5, 3]) == 8 * (2 ** 42 - 1) - 5 * 2 ** 42 + 3 * 2 ** 84


# ---------------------------------------------------------------- against the oracle
def test_statement_equals_oracle_on_an_oracle_capture(oracle):
    """fp_oracle_n8_p3 (FirstPrice, N = 8, P = 3): limb for limb."""
    d, meta, _ = load_capture("fp_oracle_n8_p3")
    for threads in (1, 16):
        o = oracle.simulate(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"], nthreads=threads)
        want = limbs(R.counters(o, d["part"], meta["P"], meta["N"]))
        assert np.array_equal(o["counters_fx"], want), threads


def test_statement_equals_oracle_on_single_participant_capture(oracle):
    """sp_oracle_n4_p1 (P = 1): nothing is charged, nobody wins, underbid regret at price 0."""
    d, meta, _ = load_capture("sp_oracle_n4_p1")
    o = oracle.simulate(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"])
    table = R.counters(o, d["part"], 1, meta["N"])
    assert np.array_equal(o["counters_fx"], limbs(table))
    assert all(row[R.N_WON] == 0 and row[R.PAID] == 0 and row[R.NET] == 0 for row in table)


def test_statement_equals_oracle_on_a_population_capture(oracle):
    """fp_dr_ts_r1024 (LR-TS allocators, DoublyRobust bidders): the slots an Oracle population never
    fills -- ALLOC_REGRET, EST_REGRET, CTR_SQERR, CTR_BIAS -- limb for limb."""
    d, meta, _ = load_capture("fp_dr_ts_r1024")
    for threads in (1, 16):
        o = oracle.simulate_pop(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"],
                                nthreads=threads, **pop_args(d, meta))
        table = R.counters(o, d["part"], meta["P"], meta["N"])
        assert np.array_equal(o["counters_fx"], limbs(table)), threads
        assert all(row[c] != 0 for row in table for c in (R.ALLOC_REGRET, R.EST_REGRET, R.CTR_SQERR, R.CTR_BIAS))


@pytest.mark.parametrize("N", [2, 4])
@pytest.mark.parametrize("name", RUNGS)
def test_ladder_statement_equals_oracle(oracle, name, N):
    """Every rung, both mechanisms, one thread and 16: the oracle's limbs are the statement's, and
    the rung meets its stated condition (the loop rung at the ladder's B here; the GPU file runs
    it at the size that makes a workgroup loop)."""
    case = ladder_case(name, N)
    for mech in (0, 1):
        first = None
        for threads in (1, 16):
            o = oracle.simulate(mech, case["items"], case["values"], case["ctx"], case["part"], case["u"],
                                nthreads=threads)
            if first is None:
                check_rung(case, o)
                first = limbs(case_statement(case, o))
            assert np.array_equal(o["counters_fx"], first), (name, N, mech, threads)
        if name == "negative":  # the totals this rung is there for: limb 2 = -1
            table = R.limbs_of(case_statement(case, o))
            assert {row[c][2] for row in table for c in range(12)} == {-1, 0}, name


def test_zero_ctr_counts_one_per_won_record(oracle):
    """The CTR-bias rule (include/auctiongym.h): a won record whose estimated CTR equals its true CTR
    bit for bit contributes exactly 1 -- 0 / 0 included -- so CTR_BIAS == N_WON for Oracle agents."""
    case = ladder_case("zero-ctr", 2)
    o = oracle.simulate(1, case["items"], case["values"], case["ctx"], case["part"], case["u"])
    table = case_statement(case, o)
    assert [row[R.CTR_BIAS] for row in table] == [row[R.N_WON] for row in table]
    assert sum(row[R.N_WON] for row in table) == B_LADDER << 36
    assert np.array_equal(o["counters_fx"][:, R.CTR_BIAS], o["counters_fx"][:, R.N_WON])


@pytest.mark.parametrize("name,mech", [("zero-ctr", 1), ("denormal-ctr", 0), ("mid", 0), ("negative", 1)])
def test_host_log_counter_terms_follow_the_statement(oracle, name, mech):
    """auctiongym_amd.Agent.log_counter_terms (the per-call path's counters of kept log records)
    on every record of a rung: its sums are the statement's, the bit-equal CTR-bias rule included
    (zero-ctr: 0 / 0 counts 1 per won record). One more set of records with est_ctr != true_ctr
    == 0: est / 0 is dropped."""
    from auctiongym_amd.Agent import C, log_counter_terms
    N = 2
    case = ladder_case(name, N)
    o = oracle.simulate(mech, case["items"], case["values"], case["ctx"], case["part"], case["u"])
    table = case_statement(case, o)
    slot = np.arange(N)[None, :] == o["winner"][:, None]
    for a in range(N):
        mine = case["part"] == a
        cols = {k: o[k][mine] for k in ("item", "value", "bid", "true_ctr", "est_ctr", "best_ev")}
        cols.update(won=slot[mine], price=np.repeat(o["price"], N)[mine.ravel()],
                    second_price=np.repeat(o["second_price"], N)[mine.ravel()])
        t = log_counter_terms(cols, True, mech == 0)
        for key in ("allocation_regret", "estimation_regret", "overbid_regret", "underbid_regret", "ctr_sqerr",
                    "ctr_bias_sum", "best_ev_sum", "n_logs", "n_won"):
            assert t[C[key]] == table[a][R.NAMES.index(key)], (name, a, key)
        if name == "zero-ctr":
            assert t[C["ctr_bias_sum"]] == t[C["n_won"]] > 0
            cols["est_ctr"] = np.full_like(cols["est_ctr"], 0.25)
            assert log_counter_terms(cols, True, False)[C["ctr_bias_sum"]] == 0
