"""The records Agent.update reads from multi-slot rounds, stated plainly: numpy, no project code.

After a round of P participants with F = min(n, P - 1) filled slots (src/Auction.py:68-74; see
tests/slots_reference.py) the participant in participant-slot s of auction i holds an
ImpressionOpportunity with
  won = (won_slot[i][s] = k >= 0),  outcome = outcome[i][k] if won else 0,
  second_price = second_price[i][k] if won else 0,
  price = log_price[i] for EVERY participant (set_price of the later slots overwrites an earlier
          winner's own price); 0.0 when F = 0 (log_price is NaN there: nobody is charged).

* LR-TS sample store (src/Agent.py:90): contexts[won], items[won], outcomes[won] -- one record
  per filled slot whose winner is an LR-TS allocator: key = agent << 16 | item << 1 | outcome[k],
  x = float32(observed context), 1.0. The rank-F participant (a click draw, no charge) is none.
* shading store (src/Bidder.py:62-63): one record per participation of a non-truthful bidder,
  utility = value * outcome[k] - log_price if won else 0, order = (first + i) * P + s.

Arrays are row-major host arrays: per (auction, participant) [B][P], per (auction, slot) [B][S].
"""
import numpy as np


def expected_records_slots(part, slot_out, bidder_kind, values, P, first):
    """The records ag_shading_collect_slots appends for auctions [first, first + B), in (auction,
    participant slot) order. slot_out: won_slot, item, gamma, est_ctr, propensity [B][P]; outcome
    [B][S]; log_price [B]. values [N][K]."""
    part = np.asarray(part)
    B = part.shape[0]
    assert part.shape == (B, P)
    i, s = np.nonzero(np.asarray(bidder_kind)[part] != 0)  # every participation of a non-truthful bidder
    a = part[i, s]
    value = np.asarray(values, np.float64)[a, slot_out["item"][i, s]]
    k = np.asarray(slot_out["won_slot"])[i, s].astype(np.int64)
    won = k >= 0
    click = np.asarray(slot_out["outcome"])[i, np.where(won, k, 0)].astype(np.float64)
    with np.errstate(invalid="ignore"):
        utility = np.where(won, value * click - np.asarray(slot_out["log_price"])[i], 0.0)
    order = (np.uint64(first) + i.astype(np.uint64)) * np.uint64(P) + s.astype(np.uint64)
    assert all(int(order[j]) == (first + int(i[j])) * P + int(s[j]) for j in (0, -1)[:len(i)])
    return dict(agent=a.astype(np.int32), gamma=slot_out["gamma"][i, s], utility=utility,
                ctr=slot_out["est_ctr"][i, s], value=value, propensity=slot_out["propensity"][i, s],
                won=won.astype(np.uint8), order=order)


def expected_lrts_samples_slots(ctx, part, slot_out, alloc_kind, OE, P):
    """The samples ag_lrts_collect_slots appends: for every filled slot k < num_filled whose winner
    is an LR-TS allocator, key = agent << 16 | item << 1 | outcome[k] and x = float32(ctx[:OE]),
    1.0f. slot_out: winner, outcome [B][S]; num_filled [B]; item [B][P].
    -> (key uint32 [n], x float32 [n][OE + 1]) in (auction, slot) order."""
    part = np.asarray(part)
    B = len(part)
    winner, F = np.asarray(slot_out["winner"]), np.asarray(slot_out["num_filled"])
    S = winner.shape[1]
    assert (F <= max(P - 1, 0)).all() and (F <= S).all()
    i, k = np.nonzero(np.arange(S)[None, :] < F[:, None])
    w = winner[i, k]
    assert ((w >= 0) & (w < P)).all()
    a = part[i, w]
    take = np.asarray(alloc_kind)[a] == 1
    key = ((a.astype(np.uint32) << 16) | (slot_out["item"][i, w].astype(np.uint32) << 1)
           | (np.asarray(slot_out["outcome"])[i, k] != 0))
    x = np.concatenate([np.asarray(ctx)[:, :OE].astype(np.float32), np.ones((B, 1), np.float32)], axis=1)[i]
    return key[take].astype(np.uint32), x[take]
