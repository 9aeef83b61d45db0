"""Agent._records builds the same ImpressionOpportunity rows from the two output layouts: the same
one-slot outcomes written once as ag_batch_out's arrays (winner, outcome, price, second_price) and
once as ag_slots_out's at max_slots = 1 (won_slot, num_filled, log_price, [1][B] per-slot arrays).
Hand-made host dicts; no GPU."""
import numpy as np
import pytest

FIELDS = ("item", "value", "bid", "best_expected_value", "true_CTR", "estimated_CTR", "price", "second_price",
          "outcome", "won")
N, K, E, B = 4, 3, 3, 5


def _layouts(P):
    g = np.random.default_rng(P)
    part = np.stack([g.choice(N, P, replace=False) for _ in range(B)], axis=1).astype(np.int32)
    per = {"item": g.integers(0, K, (P, B)).astype(np.int32), "bid": g.random((P, B)), "best_ev": g.random((P, B)),
           "true_ctr": g.random((P, B)), "est_ctr": g.random((P, B))}
    winner = g.integers(0, P, B).astype(np.int32)
    outcome = np.array([1, 0, 1, 1, 0], np.uint8)
    price, second = g.random(B) + 0.5, g.random(B)
    one = dict(per, winner=winner, outcome=outcome, price=price, second_price=second)
    charged = P >= 2  # P == 1: the kernel writes the lone bidder as winner, but nobody is charged
    won_slot = np.full((P, B), -1, np.int8)
    if charged:
        won_slot[winner, np.arange(B)] = 0
    slots = dict(per, won_slot=won_slot, num_filled=np.full(B, int(charged), np.int32),
                 log_price=price if charged else np.full(B, np.nan), winner=winner[None], outcome=outcome[None],
                 price=price[None], second_price=second[None])
    return part, one, slots, g.normal(0, 1, (E, B)), g.random((N, K)) + 0.5


@pytest.mark.parametrize("obs", [None, 2])
@pytest.mark.parametrize("P", [3, 1])
def test_records_are_equal_from_both_layouts(P, obs):
    from auctiongym_amd.Agent import _records
    part, one, slots, ctx, values = _layouts(P)
    seen = 0
    for agent in range(N):
        a = _records(part, one, ctx, agent, 0, values, obs)
        b = _records(part, slots, ctx, agent, 0, values, obs)
        assert len(a) == len(b) == int((part == agent).sum())
        seen += len(a)
        for x, y in zip(a, b):
            assert np.array_equal(x.context, y.context) and x.context.shape == ((obs or E) + 1,)
            for f in FIELDS:
                assert getattr(x, f) == getattr(y, f) and type(getattr(x, f)) is type(getattr(y, f)), f
            if P == 1:
                assert x.won is False and x.price == 0.0 and x.second_price == 0.0 and x.outcome is False
    assert seen == P * B
    if P > 1:  # the hand-made outcomes are there: every round has one winner, some clicked
        won = [r for agent in range(N) for r in _records(part, one, ctx, agent, 0, values, obs) if r.won]
        assert len(won) == B and sum(r.outcome for r in won) == 3 and all(r.price > 0 for r in won)
