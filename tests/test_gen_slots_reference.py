"""tests/gen_slots_reference.py checked on the CPU: the `slots` draw kind of the device generator
shares no counter with another draw, u_slots[0] is the auction's u, and the slot count is what
rng.integers(1, max_slots + 1) is in distribution. tests/test_gpu_generate_slots.py holds the
kernels to this statement value for value.
"""
import numpy as np
import pytest

import gen_reference as R
import gen_slots_reference as GS

SEEDS = (0, 0x9E3779B97F4A7C15)


def _collisions(calls):
    owners = {}
    for what, ctr in calls.items():
        owners.setdefault(ctr, []).append(what)
    return {c: sorted(o, key=str) for c, o in owners.items() if len(o) > 1}


def test_slot_draws_share_no_counter_at_the_widest_shape():
    """P = 64, K (OE + 1) = 64, E = 16, grids on, S = 8: every (block, stream) has one owner; the
    slot draws add the count's block (with u_slots[1]) and three more."""
    calls = GS.draw_calls(R.MAX_SLOTS, 64, 16, GS.MAX_SLOTS, grids=True)
    assert len(calls) == len(R.draw_calls(R.MAX_SLOTS, 64, 16, grids=True)) + 4
    assert _collisions(calls) == {}
    for S in range(1, GS.MAX_SLOTS + 1):
        for P in (1, 2, 16, 64):
            assert _collisions(GS.draw_calls(P, 64, 16, S)) == {}, (S, P)
    # stream 256 is above every other kind's streams
    others = {c[1] for what, c in calls.items() if what[0] != "slots"}
    assert max(others) == 255 and GS.SLOTS_STREAM == 256


def test_slot_blocks_and_words():
    """The table itself: u_slots[k] sits in block k // 2, words 2 (k % 2), + 1; k = 1 shares block 0
    with the count, whose word 1 no draw uses."""
    assert [GS.COUNTER["slots"](k) for k in range(8)] == [(k // 2, 256) for k in range(8)]
    idx = R.indices(12345, 50)
    for seed in SEEDS:
        u = GS.u_slots(seed, idx, 8)
        for k in range(1, 8):
            w = R._words(seed, idx, k // 2, 256)
            assert np.array_equal(u[k], R.uniform53(w[2 * (k % 2)], w[2 * (k % 2) + 1]))
        assert np.array_equal(GS.num_slots(seed, idx, 5),
                              1 + ((R._words(seed, idx, 0, 256)[0] * np.uint64(5)) >> np.uint64(32)))
        assert len({u[k].tobytes() for k in range(8)}) == 8  # every row its own draw


@pytest.mark.parametrize("first", [0, 2 ** 32 - 150, 5 * 10 ** 9])
def test_row_zero_is_the_auctions_uniform(first):
    idx = R.indices(first, 300)
    for seed in SEEDS:
        for S in (1, 2, 8):
            assert np.array_equal(GS.u_slots(seed, idx, S)[0], R.uniforms(seed, idx))


def test_num_slots_range_and_extreme_words():
    for S in range(1, GS.MAX_SLOTS + 1):
        assert GS.count_of_word(0, S) == 1
        assert GS.count_of_word(2 ** 32 - 1, S) == S
        # the boundaries between counts: the first word that gives n + 1
        for n in range(1, S):
            w = -(-(n << 32) // S)
            assert GS.count_of_word(w, S) == n + 1 and GS.count_of_word(w - 1, S) == n
        for seed in SEEDS:
            ns = GS.num_slots(seed, R.indices(2 ** 32 - 150, 4000), S)
            assert ns.dtype == np.int32 and ns.min() >= 1 and ns.max() <= S
            assert S > 1 or (ns == 1).all()


@pytest.mark.parametrize("S", [2, 3, 8])
@pytest.mark.parametrize("seed", SEEDS)
def test_num_slots_is_uniform_over_one_to_S(seed, S):
    """2^16 consecutive indices: each count's frequency within 5 standard deviations of 1 / S
    (a binomial's sd, sqrt(p (1 - p) / n))."""
    n = 1 << 16
    ns = GS.num_slots(seed, R.indices(0, n), S)
    freq = np.bincount(ns, minlength=S + 1)[1:] / n
    sd = np.sqrt((1 / S) * (1 - 1 / S) / n)
    assert len(freq) == S and np.abs(freq - 1 / S).max() < 5 * sd, (freq, sd)


def test_u_slots_are_53_bit_uniforms():
    for seed in SEEDS:
        u = GS.u_slots(seed, R.indices(5 * 10 ** 9, 5000), 8)
        assert u.shape == (8, 5000) and u.dtype == np.float64
        assert (u >= 0).all() and (u < 1).all()
        k = u * 2.0 ** 53
        assert np.array_equal(k, np.floor(k))  # a multiple of 2^-53
        assert abs(u[1:].mean() - 0.5) < 5 * np.sqrt(1 / 12 / u[1:].size)
