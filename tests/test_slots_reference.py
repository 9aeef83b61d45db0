"""tests/slots_reference.py (the multi-slot semantics in plain numpy and Python integers) pinned to
the reference's own multi-slot runs (tests/golden/make_golden_slots.py): every log field, allocate's
arrays, the utilities, regrets and the revenue. At one slot it is pinned to the oracle on existing
captures, and the oracle's per-participant fields are pinned to the fixtures': the oracle's
per-participant outputs plus slots_reference give the expected multi-slot result of any population.
"""
import numpy as np
import pytest

import slots_reference as SR
from conftest import load_capture, mech_code, pop_args
from counter_reference import (ALLOC_REGRET, EST_REGRET, GROSS, NET, N_LOGS, OVERBID, PAID, UNDERBID, limbs_of)
from slots_cases import (FIELDS, ORACLE_SLOT_CAPTURES, POP_SLOT_CAPTURES, SLOT_CAPTURES, capture, fixture_expected)

S36 = 2.0 ** -36


def test_ranking_is_stable_descending():
    assert SR.ranking([1.0, 3.0, 3.0, 2.0, 3.0]) == [1, 2, 4, 3, 0]
    assert SR.ranking([0.5]) == [0]
    assert SR.ranking([2.0, 2.0]) == [0, 1]


@pytest.mark.parametrize("P,n,F,cons", [(1, 1, 0, 1), (1, 2, 0, 1), (2, 1, 1, 1), (2, 3, 1, 2), (3, 2, 2, 2),
                                        (3, 8, 2, 3), (4, 3, 3, 3), (9, 8, 8, 8)])
def test_filled_and_consumed(P, n, F, cons):
    assert SR.filled(n, P) == F and SR.consumed(n, P) == cons
    bids = np.arange(P, 0, -1).astype(float)
    for mech in (SR.FIRST_PRICE, SR.SECOND_PRICE):
        w, p, s = SR.allocate(mech, bids, n)
        assert len(w) == min(n, P) and len(s) == min(n, P - 1)
        assert len(p) == (min(n, P) if mech == SR.FIRST_PRICE else min(n, P - 1))
        assert min(len(w), len(p), len(s)) == F


def test_binomial1_is_numpys_inversion():
    """Against numpy itself: binomial(1, p) and the double it consumes, from cloned generators."""
    g = np.random.default_rng(5)
    ps = np.concatenate([g.random(4000), [0.0, 0.5, 1.0, 1e-300, 1.0 - 2.0 ** -53]])
    for p in ps:
        a = np.random.default_rng(int(g.integers(1 << 30)))
        b = np.random.Generator(np.random.PCG64())
        b.bit_generator.state = a.bit_generator.state
        got = int(a.binomial(1, p))
        u = b.random() if p != 0.0 else 0.0
        assert got == SR.binomial1(float(p), u)
        assert a.bit_generator.state == b.bit_generator.state  # nothing drawn for p == 0


@pytest.mark.parametrize("name", SLOT_CAPTURES)
def test_reference_pins_every_log_field(name):
    d, meta, agg = capture(name)
    e = fixture_expected(name)
    P, S = meta["P"], meta["max_slots"]
    assert set(np.unique(d["num_slots"])) == set(range(1, S + 1))  # every n drawn, n >= P included
    assert np.array_equal(e["log_price_slot"], d["slot_price"])
    assert np.array_equal(e["log_second"], d["slot_second_price"])
    assert np.array_equal(e["log_outcome"], d["outcome"].astype(bool))
    assert np.array_equal(e["log_won"], d["won"].astype(bool))
    assert np.array_equal(e["num_filled"], np.minimum(d["num_slots"], P - 1))
    # the doubles consumed: min(n, P) per round, NaN beyond
    assert np.array_equal(np.isfinite(d["u_slots"]).sum(axis=1), np.minimum(d["num_slots"], P))
    w, p, s = SR.allocate_padded(mech_code(meta), d["slot_bid"], d["num_slots"], S)
    assert np.array_equal(w, d["alloc_winner"])
    assert np.array_equal(p, d["alloc_price"], equal_nan=True)
    assert np.array_equal(s, d["alloc_second"], equal_nan=True)
    # the filled slots are allocate's first F
    for k in range(S):
        f = k < e["num_filled"]
        assert np.array_equal(e["winner"][f, k], d["alloc_winner"][f, k]) and (e["winner"][~f, k] == -1).all()
        assert np.array_equal(e["price"][f, k], d["alloc_price"][f, k]) and np.isnan(e["price"][~f, k]).all()
    cnt = np.array(e["counters"], dtype=object).astype(float) * S36
    rt = dict(rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(cnt[:, NET], agg["net_utility"], **rt)
    np.testing.assert_allclose(cnt[:, GROSS], agg["gross_utility"], **rt)
    np.testing.assert_allclose(cnt[:, ALLOC_REGRET], agg["allocation_regret"], **rt)
    np.testing.assert_allclose(cnt[:, EST_REGRET], agg["estimation_regret"], **rt)
    np.testing.assert_allclose(cnt[:, OVERBID], agg["overbid_regret"], **rt)
    np.testing.assert_allclose(cnt[:, UNDERBID], agg["underbid_regret"], **rt)
    np.testing.assert_allclose(cnt[:, N_LOGS], agg["n_logs"], **rt)
    np.testing.assert_allclose(e["revenue"] * S36, agg["revenue"], **rt)
    assert e["revenue"] == sum(int(t[PAID]) for t in e["counters"])


def test_overbid_is_nonzero_under_second_price_with_several_slots():
    """The one-slot shortcut (no OVERBID term under SecondPrice) does not hold: an earlier winner
    logs the last filled slot's price against its own second price."""
    d, meta, agg = capture("slots_sp_oracle_p4_s3")
    assert any(v < 0.0 for v in agg["overbid_regret"])
    e = fixture_expected("slots_sp_oracle_p4_s3")
    assert any(t[OVERBID] < 0 for t in e["counters"])


@pytest.mark.parametrize("name", ORACLE_SLOT_CAPTURES)
def test_oracle_fields_equal_fixture_oracle(oracle, name):
    d, meta, _ = capture(name)
    o = oracle.simulate(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], np.nan_to_num(d["u_slots"][:, 0]))
    for k in FIELDS:
        assert np.array_equal(o[k], d["slot_" + k]), k
    assert np.array_equal(o["item"], d["item"])


@pytest.mark.parametrize("name", POP_SLOT_CAPTURES)
def test_oracle_fields_equal_fixture_population(oracle, name):
    d, meta, _ = capture(name)
    o = oracle.simulate_pop(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"],
                            np.nan_to_num(d["u_slots"][:, 0]), **pop_args(d, meta))
    for k in FIELDS:
        assert np.array_equal(o[k], d["slot_" + k]), k
    assert np.array_equal(o["item"], d["item"])
    if "Empirical" in meta["bidders"][0]:
        assert np.array_equal(o["gamma"], d["slot_gamma"])


@pytest.mark.parametrize("name,pop", [("sp_oracle_r4096", False), ("fp_oracle_n8_p3", False),
                                      ("fp_empirical_r2048", True)])
def test_one_slot_equals_the_oracle(oracle, name, pop):
    """max_slots = 1 on existing captures: outputs and every counter limb equal the oracle's."""
    d, meta, _ = load_capture(name)
    mech = mech_code(meta)
    if pop:
        o = oracle.simulate_pop(mech, d["items"], d["values"], d["ctx"], d["part"], d["u"], **pop_args(d, meta))
    else:
        o = oracle.simulate(mech, d["items"], d["values"], d["ctx"], d["part"], d["u"])
    B = len(d["u"])
    e = SR.simulate(mech, o, d["part"], np.ones(B, np.int32), d["u"].reshape(B, 1), 1, N=meta["N"])
    assert np.array_equal(e["winner"][:, 0], o["winner"])
    assert np.array_equal(e["price"][:, 0], o["price"])
    assert np.array_equal(e["second_price"][:, 0], o["second_price"])
    assert np.array_equal(e["outcome"][:, 0], o["outcome"])
    assert np.array_equal(np.array(limbs_of(e["counters"]), np.int64), o["counters_fx"])
