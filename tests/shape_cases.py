"""Capture names and case tables of the off-catalogue-shape tests (tests/test_oracle_shapes.py,
tests/test_gpu_shapes.py) and of `tests/golden/make_golden.py --only shapes`, which writes the
captures. Plain data: no fixtures, no pytest hooks.

The catalogue shape every other fixture has is K = 12, E = 5, OE = 4 (D = E + 1 = 6, LR-TS width
OE + 1 = 5). Everything here is another shape.
"""

ROUNDS = 256  # reference rounds per capture

# Oracle + truthful populations: name -> (N, K, E, OE, P, allocation, config seed)
# Pinned: numpy's dot order is restated for K >= 2 with D <= 7 or K % 4 == 0 (Auction.py), so
# every field of these equals the reference's bit for bit.
ORACLE_PINNED = {
    "shape_sp_n4_k3_e2_p2": (4, 3, 2, 1, 2, "SecondPrice", 31),
    "shape_fp_n5_k7_e3_p3": (5, 7, 3, 2, 3, "FirstPrice", 32),
    "shape_sp_n6_k16_e7_p4": (6, 16, 7, 4, 4, "SecondPrice", 33),
    "shape_fp_n6_k17_e4_p2": (6, 17, 4, 4, 2, "FirstPrice", 34),
    "shape_sp_n4_k8_e10_p2": (4, 8, 10, 4, 2, "SecondPrice", 35),
    "shape_sp_n10_k12_e1_p9": (10, 12, 1, 1, 9, "SecondPrice", 36),
}
# Unpinned catalogue shapes (K = 1; D = 8 with K % 4 != 0): numpy takes a dot kernel whose
# summation order is not restated -- true_ctr to a bound, item / winner / outcome exact.
ORACLE_UNPINNED = {
    "shape_sp_n4_k1_e5_p2": (4, 1, 5, 4, 2, "SecondPrice", 37),
    "shape_fp_n6_k10_e7_p2": (6, 10, 7, 4, 2, "FirstPrice", 38),
}

# General populations: name -> (reference config, K, E, OE)
POP_PINNED = {
    "shape_sp_ts_k9_e4_oe4": ("SP_Truthful_TS.json", 9, 4, 4),   # LR-TS width 5 off the catalogue shape
    "shape_fp_dr_ts_k9_e4_oe4": ("FP_DR_TS.json", 9, 4, 4),      # first (uninitialised) iteration
}
# LR-TS width 3: torch's sgemv sums in an order pinned for width 5 only -- est_ctr / bid / price to
# a bound, true_ctr / best_ev / item / winner / outcome exact.
POP_UNPINNED = {
    "shape_sp_ts_k7_e3_oe2": ("SP_Truthful_TS.json", 7, 3, 2),
}

# Relative bounds of the unpinned captures' inexact fields: 4 x the oracle-vs-reference deviation
# measured on the committed fixture (the figures are in tests/test_oracle_shapes.py's docstrings).
UNPINNED_BOUNDS = {
    "shape_sp_n4_k1_e5_p2": {"true_ctr": 4 * 1.797848214450528e-15},
    "shape_fp_n6_k10_e7_p2": {"true_ctr": 4 * 7.531184734750154e-16},
    "shape_sp_ts_k7_e3_oe2": {"est_ctr": 4 * 2.823910805835894e-07, "bid": 4 * 2.8239108050861674e-07,
                              "price": 4 * 2.8239108050861674e-07},
}

# ---- general populations (LR-TS allocators, shading bidders) at D != 6 or LR-TS width != 5 ----
# (E, OE): D = E + 1 in 2..8, LR-TS width OE + 1 in {2, 3, 4, 5, 7, 8}; (4, 4) has width 5 at
# D = 5 and (5, 3) has D = 6 at width 4 -- neither is the shipped shape, so the compile-time-width
# build must not be taken.
GENERAL_SHAPES = ((1, 1), (2, 1), (3, 2), (4, 4), (6, 3), (7, 6), (7, 7), (5, 3))
_PS = (1, 2, 3, 8)
_KS = (3, 7, 16)
_BS = (1, 255, 2 * 256 + 37)     # 256-lane builds: one lane, one ragged tile, several tiles + a tail
B_LARGE = 2 * 1024 + 37          # 1024-lane builds


def _general_cases():
    """The table of test_gpu_shapes.test_general_population: one row per k_simulate build a general
    population can reach -- (population, item search, lanes) per D -- with P, K, the mechanism,
    Thompson sampling and B cycling at strides that pair every value of one axis with every value
    of the others, then the rows for the launch cap, ragged item counts, the compact noise
    layout, the automatic workgroup size and K = 12."""
    rows = []
    for s, (E, OE) in enumerate(GENERAL_SHAPES):
        for r, (pop, exact, bt) in enumerate((("ts", False, 256), ("ts", True, 256), ("all", False, 256),
                                              ("all", True, 256), ("all", False, 1024))):
            rows.append(dict(E=E, OE=OE, K=17 if exact else _KS[(s + r) % 3], P=_PS[(s + r) % 4], pop=pop,
                             bt=bt, mech=(s + r // 2) % 2, sample=(s + r) % 2 == 0,
                             B=B_LARGE if bt == 1024 else _BS[(s + 2 * r) % 3], cap=0, ragged=False,
                             compact=False))
    base = dict(cap=0, ragged=False, compact=False, sample=True, mech=0)
    rows += [
        dict(base, E=3, OE=2, K=7, P=2, pop="ts", bt=256, B=_BS[2], cap=300),            # several ragged launches
        dict(base, E=6, OE=3, K=16, P=3, pop="all", bt=1024, B=B_LARGE, cap=300, mech=1),
        dict(base, E=2, OE=1, K=7, P=3, pop="all", bt=256, B=_BS[2], ragged=True),       # set_agent_items
        dict(base, E=7, OE=6, K=3, P=2, pop="all", bt=256, B=_BS[2], compact=True),      # compact noise
        dict(base, E=3, OE=2, K=16, P=8, pop="ts", bt=1024, B=B_LARGE, compact=True, mech=1),
        dict(base, E=1, OE=1, K=16, P=8, pop="all", bt=0, B=_BS[2]),                     # automatic lanes
        dict(base, E=7, OE=7, K=17, P=1, pop="ts", bt=0, B=_BS[1], mech=1),
        dict(base, E=5, OE=3, K=12, P=2, pop="all", bt=256, B=_BS[2]),                   # K = 12: D = 6 alone
        dict(base, E=4, OE=4, K=12, P=8, pop="ts", bt=256, B=_BS[2], mech=1),            # K = 12: width 5 alone
        dict(base, E=2, OE=1, K=7, P=4, pop="all", bt=256, B=_BS[2]),                    # P in 4..7: one D each
        dict(base, E=3, OE=2, K=16, P=5, pop="ts", bt=256, B=_BS[1], mech=1),
        dict(base, E=6, OE=3, K=3, P=6, pop="all", bt=1024, B=B_LARGE, sample=False),
        dict(base, E=7, OE=7, K=17, P=7, pop="all", bt=256, B=_BS[2], mech=1),
    ]
    return rows


GENERAL_CASES = _general_cases()


def general_build(case):
    """The k_simulate build ag_simulate launches for a GENERAL_CASES row, as (D, G, PRUNE, BT):
    the dispatch rules of simulate_general (csrc/ag_kernels.hip) and pick_kernel_for
    (csrc/ag_sim_p.hip) restated for P <= 8. "ship" instead of G where the compile-time-width
    build of the shipped shape would be taken; None where the workgroup size is chosen by the
    population's LDS image (bt = 0) or the launch is refused."""
    D, width = case["E"] + 1, case["OE"] + 1
    prune = D <= 8 and case["K"] <= 16            # AG_ITEM_SEARCH_AUTO, positive catalogue values
    G = "truthful" if case["pop"] == "ts" else "all"
    if prune and D == 6 and width == 5:
        G = "ship"
    if case["bt"] == 0:
        return None
    if case["bt"] == 1024:
        if not prune:
            return None                           # refused: 1024 lanes come with the screen
        if G != "ship":
            G = "all"                             # no TruthfulBidder-only build in 1024 lanes
    return (D, G, prune, case["bt"])


def general_builds_shipped():
    """Every (D, G, PRUNE, BT) pick_kernel_for returns for a general population that is not the
    shipped shape (the runtime-width builds; the same set for every P in 1..8)."""
    return {(D, G, prune, 256) for D in range(2, 9) for G in ("truthful", "all") for prune in (True, False)} | \
           {(D, "all", True, 1024) for D in range(2, 9)}


# an unpinned capture's field -> the reference array it is compared with
REF_FIELD = {"true_ctr": "slot_true_ctr", "est_ctr": "slot_est_ctr", "bid": "slot_bid", "price": "price"}


def within_bound(got, ref, bound):
    """max |got - ref| / |ref| <= bound over the entries that are not NaN in both."""
    import numpy as np
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    both_nan = np.isnan(got) & np.isnan(ref)
    rel = np.abs(got - ref)[~both_nan] / np.abs(ref[~both_nan])
    worst = float(rel.max()) if rel.size else 0.0
    return worst <= bound, worst
