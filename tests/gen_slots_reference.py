"""A plain statement of the device generator's draws for multi-slot rounds (csrc/ag_philox.h
gen_num_slots / gen_u_slot, k_generate_slots, the SLOTS builds' generate mode), in numpy.

Test helper, not a conftest. Nothing here calls project code: Philox, the 53-bit uniform and the
index arithmetic come from tests/gen_reference.py, and this adds the one draw kind `slots`:

  kind    stream   blocks
  slots   256      0: word 0 -> the slot count, words 2-3 -> u_slots[1] (word 1 unused);
                   k // 2 for u_slots[k], k = 2..7: words 2 (k % 2), 2 (k % 2) + 1

u_slots[0] is the auction's u (kind `uniform`: stream 0, block 0, words 0-1), so a generated
multi-slot batch has exactly the ctx, part and u of the one-slot batch of the same (seed, first, B).
"""
import numpy as np

import gen_reference as G

MAX_SLOTS = 8                  # AG_MAX_SLOTS
SLOTS_STREAM = 256             # the first stream above the grids' 204..255
STREAM = dict(G.STREAM, slots=SLOTS_STREAM)
COUNTER = dict(G.COUNTER, slots=lambda k: (k // 2, SLOTS_STREAM))  # k = 0: the count's block


def draw_calls(P, KDo, E, S, grids=True):
    """gen_reference.draw_calls plus the slot draws of a round with max_slots = S: the count
    (with u_slots[1], block 0) and a block for every later pair of uniforms."""
    calls = G.draw_calls(P, KDo, E, grids=grids, counter=COUNTER)
    calls[("slots", "count+u1")] = COUNTER["slots"](0)
    assert S < 2 or COUNTER["slots"](1) == COUNTER["slots"](0)
    for k in range(2, S):
        calls[("slots", "u", k // 2)] = COUNTER["slots"](k)
    return calls


def count_of_word(w0, S):
    """The slot count from word 0: the participant picks' multiply-shift, 1..S."""
    return (1 + ((np.asarray(w0, np.uint64) * np.uint64(S)) >> np.uint64(32))).astype(np.int32)


def num_slots(seed, idx, S):
    """int32 [B] in 1..S (rng.integers(1, max_slots + 1) in distribution)."""
    return count_of_word(G._words(seed, idx, *COUNTER["slots"](0))[0], S)


def u_slots(seed, idx, S):
    """float64 [S][B]: row 0 the auction's u, row k >= 1 the 53-bit uniform of words 2 (k % 2),
    2 (k % 2) + 1 of block k // 2 of stream 256."""
    idx = np.asarray(idx, np.uint64)
    u = np.empty((S, idx.size))
    u[0] = G.uniforms(seed, idx)
    for k in range(1, S):
        w = G._words(seed, idx, *COUNTER["slots"](k))
        u[k] = G.uniform53(w[2 * (k % 2)], w[2 * (k % 2) + 1])
    return u
