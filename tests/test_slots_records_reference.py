"""tests/slots_records_reference.py pinned to the reference's own logs, without a GPU.

The statement runs on the multi-slot fixtures' per-round results (tests/slots_reference.py over
the fixture's own per-participant fields, itself pinned by tests/test_slots_reference.py) and must
give what the reference's Agent.update reads from its logs: the EmpiricalShadedBidder's gammas,
won flags and utilities value * outcome - price, and the LR-TS allocators' won (context, item,
outcome) samples.

The fixtures are also asserted to hold the cases the collectors can get wrong:
  * an auction with two or more winners that are learners (several records of one lane): every
    agent of slots_sp_ts_p3_s3 is an LR-TS allocator, every agent of slots_fp_empirical_p3_s3 an
    EmpiricalShadedBidder;
  * an earlier-slot winner whose logged price is not its own price_k;
  * an auction with n >= P (the rank-F participant draws a click and is no record).
"""
from collections import Counter

import numpy as np
import pytest

import slots_records_reference as RR
from conftest import pop_args
from slots_cases import capture, fixture_expected

EMPIRICAL, TS = "slots_fp_empirical_p3_s3", "slots_sp_ts_p3_s3"


def fixture_slot_out(name):
    """The fixture's rounds as row-major ag_slots_out arrays: the per-slot and per-round results of
    slots_reference.simulate, the per-participant fields the reference logged."""
    d, meta, _ = capture(name)
    exp = fixture_expected(name)
    out = {k: exp[k] for k in ("winner", "outcome", "num_filled", "log_price", "won_slot", "price")}
    out.update(item=d["item"], gamma=d["slot_gamma"], est_ctr=d["slot_est_ctr"],
               propensity=np.full(d["part"].shape, np.nan))
    return out


def lrts_rows(key, x):
    """(key, x-row) records as sorted rows of uint32 words: a multiset."""
    rows = np.concatenate([np.asarray(key).view(np.uint32)[:, None],
                           np.ascontiguousarray(x, np.float32).view(np.uint32)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_empirical_logs(recs, name, what):
    """Shading records (sorted by order) of the fixture against the reference's logs, per agent in log
    order: gamma, won and utility = value * outcome - slot_price where won, else 0, bit for bit; all
    64 bits of order."""
    d, meta, _ = capture(name)
    bk = pop_args(d, meta)["bid_kind"]
    P = meta["P"]
    idx = np.argsort(recs["order"], kind="stable")
    recs = {f: np.asarray(v)[idx] for f, v in recs.items()}
    r, s = np.nonzero(bk[d["part"]] != 0)
    assert len(r) > 0 and len(recs["order"]) == len(r), what
    assert np.array_equal(recs["order"], r.astype(np.uint64) * np.uint64(P) + s.astype(np.uint64)), what
    assert np.array_equal(recs["agent"], d["part"][r, s]), what
    won = d["won"][r, s].astype(bool)
    util = np.where(won, d["slot_value"][r, s] * d["outcome"][r, s].astype(np.float64) - d["slot_price"][r, s], 0.0)
    assert np.array_equal(_bits(recs["gamma"]), _bits(d["slot_gamma"][r, s])), what
    assert np.array_equal(recs["won"].astype(bool), won), what
    assert np.array_equal(_bits(recs["utility"]), _bits(util)), what
    assert np.array_equal(_bits(recs["value"]), _bits(d["slot_value"][r, s])), what
    assert won.any() and (util != 0).any()


def check_lrts_logs(key, x, name, what):
    """LR-TS samples of the fixture against its won records: per agent the multiset of (float32
    observed context + 1, item, outcome)."""
    d, meta, _ = capture(name)
    ak = pop_args(d, meta)["alloc_kind"]
    OE = meta["OE"]
    r, s = np.nonzero(d["won"].astype(bool) & (ak[d["part"]] == 1))
    a = d["part"][r, s].astype(np.uint32)
    want_key = (a << 16) | (d["item"][r, s].astype(np.uint32) << 1) | (d["outcome"][r, s] != 0)
    want_x = np.concatenate([d["ctx"][r, :OE].astype(np.float32), np.ones((len(r), 1), np.float32)], axis=1)
    assert len(r) > 0 and len(key) == len(r), (what, len(key), len(r))
    for agent in np.unique(a):
        g, w = (np.asarray(key) >> 16) == agent, a == agent
        assert np.array_equal(lrts_rows(np.asarray(key)[g], np.asarray(x)[g]), lrts_rows(want_key[w], want_x[w])), \
            (what, int(agent))


def test_shading_records_equal_the_reference_logs():
    d, meta, _ = capture(EMPIRICAL)
    bk = pop_args(d, meta)["bid_kind"]
    recs = RR.expected_records_slots(d["part"], fixture_slot_out(EMPIRICAL), bk, d["values"], meta["P"], 0)
    assert set(recs["agent"]) == set(range(meta["N"])) and (bk == 1).all()  # every agent shades
    check_empirical_logs(recs, EMPIRICAL, "statement")


def test_lrts_samples_equal_the_reference_logs():
    d, meta, _ = capture(TS)
    ak = pop_args(d, meta)["alloc_kind"]
    key, x = RR.expected_lrts_samples_slots(d["ctx"], d["part"], fixture_slot_out(TS), ak, meta["OE"], meta["P"])
    check_lrts_logs(key, x, TS, "statement")
    # a TruthfulBidder-only population has no shading record
    bk = pop_args(d, meta)["bid_kind"]
    assert len(RR.expected_records_slots(d["part"], fixture_slot_out(TS), bk, d["values"], meta["P"], 0)["order"]) == 0


def fixture_conditions(name):
    """(auctions with >= 2 learner winners, earlier-slot winners whose logged price is not their own
    price_k, auctions with n >= P) of a fixture."""
    d, meta, _ = capture(name)
    pa = pop_args(d, meta)
    learner = (pa["alloc_kind"] == 1) | (pa["bid_kind"] != 0)
    won = d["won"].astype(bool)
    two = int(((won & learner[d["part"]]).sum(axis=1) >= 2).sum())
    exp = fixture_expected(name)
    own = np.take_along_axis(exp["price"], np.maximum(exp["won_slot"], 0).astype(np.int64), axis=1)
    overwritten = int((won & (d["slot_price"] != own)).sum())
    assert np.array_equal(exp["won_slot"] >= 0, won)
    return two, overwritten, int((d["num_slots"] >= meta["P"]).sum())


@pytest.mark.parametrize("name", [EMPIRICAL, TS])
def test_fixtures_hold_the_cases(name):
    two, overwritten, n_ge_p = fixture_conditions(name)
    assert two > 100, two
    assert overwritten > 50, overwritten
    assert n_ge_p > 100, n_ge_p
    # an overwritten price is a LATER slot's: the winner is not in the last filled slot
    exp = fixture_expected(name)
    k = exp["won_slot"]
    assert ((k >= 0) & (k < exp["num_filled"][:, None] - 1)).any()


def test_statement_counts():
    """One LR-TS record per filled slot won by an LR-TS agent, one shading record per participation."""
    d, meta, _ = capture(TS)
    exp = fixture_expected(TS)
    key, _ = RR.expected_lrts_samples_slots(d["ctx"], d["part"], fixture_slot_out(TS), np.ones(meta["N"], np.int32),
                                            meta["OE"], meta["P"])
    assert len(key) == int(exp["num_filled"].sum()) == int(d["won"].sum())
    per_auction = Counter(np.minimum(d["num_slots"], meta["P"] - 1).tolist())
    assert per_auction[2] > 0 and max(per_auction) == meta["P"] - 1
