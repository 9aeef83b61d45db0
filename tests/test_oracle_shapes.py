"""The oracle pinned against the reference at shapes other than the catalogue shape
(K = 12, E = 5, OE = 4) that every fixture of tests/test_oracle_golden.py has. CPU only.

The captures (tests/shape_cases.py; written by `make_golden.py --only shapes`, 256 reference
rounds each) come in two kinds. The pinned ones -- K >= 2 with D = E + 1 <= 7 or K % 4 == 0, and
LR-TS models of width OE + 1 = 5 -- pass the very assertions of test_oracle_golden.py: every field
bit for bit. The unpinned ones (K = 1; D = 8 with K % 4 != 0; LR-TS width 3) are the shapes the
drop-in warns about: numpy and torch take summation orders there that the oracle does not restate,
so the discrete results are exact and the affected floats are held to 4 x the deviation measured
on the committed fixture.
"""
import warnings

import numpy as np
import pytest

import test_oracle_golden as G
from conftest import load_capture, mech_code, pop_args
from shape_cases import (ORACLE_PINNED, ORACLE_UNPINNED, POP_PINNED, POP_UNPINNED, REF_FIELD, UNPINNED_BOUNDS,
                         within_bound)


def test_fixture_shapes_are_what_the_tables_say():
    for name, (N, K, E, OE, P, alloc, seed) in {**ORACLE_PINNED, **ORACLE_UNPINNED}.items():
        d, meta, _ = load_capture(name)
        assert (meta["N"], meta["K"], meta["E"], meta["OE"], meta["P"], meta["allocation"]) == (N, K, E, OE, P, alloc)
        assert d["items"].shape == (N, K, E + 1) and d["ctx"].shape == (256, E) and d["part"].shape == (256, P)
    for name, (cfg, K, E, OE) in {**POP_PINNED, **POP_UNPINNED}.items():
        d, meta, _ = load_capture(name)
        assert (meta["K"], meta["E"], meta["OE"], meta["ts_dim"]) == (K, E, OE, OE + 1)
        assert d["ts_noise"].shape == (256, meta["P"], K, OE + 1) and d["ts_m"].shape == (meta["N"], K, OE + 1)


@pytest.mark.parametrize("name", ORACLE_PINNED)
def test_simulate_matches_reference_bitwise(oracle, name):
    G.test_simulate_matches_reference_bitwise(oracle, name)


@pytest.mark.parametrize("name", ORACLE_PINNED)
def test_counters_match_reference_aggregates(oracle, name):
    G.test_counters_match_reference_aggregates(oracle, name)


@pytest.mark.parametrize("name", POP_PINNED)
def test_population_matches_reference(oracle, name):
    G.test_population_matches_reference(oracle, name)


@pytest.mark.parametrize("name", ORACLE_UNPINNED)
def test_unpinned_catalogue_shapes(oracle, name):
    """K = 1 (numpy's ddot) and D = 8, K = 10 (a remainder kernel of dgemv_t): item, value, winner
    and outcome equal the reference's; true_ctr (= est_ctr for an OracleAllocator) within 4 x the
    deviation measured on the committed fixture --
      shape_sp_n4_k1_e5_p2:  measured 1.797848214450528e-15 relative (36 % of entries differ),
                             bound 7.191392857802112e-15;
      shape_fp_n6_k10_e7_p2: measured 7.531184734750154e-16 relative (7 % of entries differ),
                             bound 3.0124738939000616e-15."""
    d, meta, _ = load_capture(name)
    o = oracle.simulate(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"])
    assert np.array_equal(o["item"], d["item"])
    assert np.array_equal(o["value"], d["slot_value"])
    assert np.array_equal(o["winner"], d["winner"])
    assert np.array_equal(o["outcome"], d["outcome"])
    bound = UNPINNED_BOUNDS[name]["true_ctr"]
    for f in ("true_ctr", "est_ctr"):
        ok, worst = within_bound(o[f], d["slot_" + f], bound)
        print(name, f, "relative deviation", worst, "bound", bound)
        assert ok, (f, worst, bound)


@pytest.mark.parametrize("name", POP_UNPINNED)
def test_unpinned_lrts_width(oracle, name):
    """LR-TS models of width OE + 1 = 3 (E = 3, K = 7): item, winner, outcome, true_ctr and
    best_ev equal the reference's bit for bit; est_ctr, bid and price within 4 x the deviation
    measured on the committed fixture --
      est_ctr: measured 2.823910805835894e-07 relative (5 % of entries differ), bound 1.1295643223343576e-06;
      bid, price: measured 2.8239108050861674e-07, bound 1.129564322034467e-06."""
    d, meta, _ = load_capture(name)
    o = oracle.simulate_pop(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"],
                            **pop_args(d, meta))
    for f, ref in (("item", "item"), ("winner", "winner"), ("outcome", "outcome"), ("true_ctr", "slot_true_ctr"),
                   ("best_ev", "slot_best_ev")):
        assert np.array_equal(o[f], d[ref]), f
    for f, bound in UNPINNED_BOUNDS[name].items():
        ok, worst = within_bound(o[f], d[REF_FIELD[f]], bound)
        print(name, f, "relative deviation", worst, "bound", bound)
        assert ok, (f, worst, bound)


def test_unpinned_shapes_warn():
    """The drop-in warns where parity is unpinned: the catalogue shapes of ORACLE_UNPINNED (and no
    pinned one), and an LR-TS allocator of a width other than 5 -- once per width."""
    from auctiongym_amd import BidderAllocation as BA
    from auctiongym_amd.Auction import warn_unpinned_catalogue
    for N, K, E, *_ in ORACLE_UNPINNED.values():
        with pytest.warns(UserWarning, match=rf"catalogue shape K={K}, E\+1={E + 1}: .* unpinned"):
            warn_unpinned_catalogue(K, E + 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for N, K, E, *_ in list(ORACLE_PINNED.values()) + [(6, 12, 5)]:
            warn_unpinned_catalogue(K, E + 1)
    BA._warned_widths.clear()
    with pytest.warns(UserWarning, match=r"LR-TS model width OE\+1=3: .* unpinned") as rec:
        BA.PyTorchLogisticRegressionAllocator(None, 2, 7)
        BA.PyTorchLogisticRegressionAllocator(None, 2, 9)
    assert len([w for w in rec if "LR-TS model width" in str(w.message)]) == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        BA.PyTorchLogisticRegressionAllocator(None, 4, 12)  # the pinned width
        BA.PyTorchLogisticRegressionAllocator(None, 2, 7)   # already warned
    BA._warned_widths.clear()
