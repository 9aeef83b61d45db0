"""The multi-slot fixtures (tests/golden/make_golden_slots.py) and what the tests share about them."""
import functools

from conftest import load_capture, mech_code

ORACLE_SLOT_CAPTURES = tuple(f"slots_{m}_oracle_p{P}_s{S}" for (P, S) in ((4, 3), (2, 3), (3, 8), (1, 2))
                             for m in ("fp", "sp"))
POP_SLOT_CAPTURES = ("slots_fp_empirical_p3_s3", "slots_sp_ts_p3_s3")
SLOT_CAPTURES = ORACLE_SLOT_CAPTURES + POP_SLOT_CAPTURES
FIELDS = ("value", "bid", "est_ctr", "true_ctr", "best_ev")


@functools.lru_cache(maxsize=None)
def capture(name):
    """(arrays, meta, aggregates) of a fixture; loaded once, shared, never written to."""
    d, meta, agg = load_capture(name)
    for v in d.values():
        v.setflags(write=False)
    return d, meta, agg


def fixture_fields(d):
    return {k: d["slot_" + k] for k in FIELDS}


@functools.lru_cache(maxsize=None)
def fixture_expected(name):
    """slots_reference.simulate over the fixture's own per-participant fields."""
    import slots_reference as SR
    d, meta, _ = capture(name)
    return SR.simulate(mech_code(meta), fixture_fields(d), d["part"], d["num_slots"], d["u_slots"],
                       meta["max_slots"], N=meta["N"])
