"""Multi-slot rounds, stated plainly: numpy and Python integers, no project code.

What src/Auction.py:28-74 does with a round of P participants and n = rng.integers(1, max_slots + 1)
slots, given each participant's bid, value, true and estimated CTR and best expected value (the
oracle's per-participant outputs do not depend on the number of slots):

* ranking: descending bid, ties to the lower participant slot (a stable order);
* allocate (src/AuctionAllocation.py:18-35): winners = ranking[:n]; FirstPrice prices =
  sorted[:n], second prices = sorted[1:n + 1]; SecondPrice both = sorted[1:n + 1];
* rng.binomial(1, CTRs[winners]) consumes one double per winner, min(n, P) of them, in rank order
  (numpy's inversion sampler for n = 1, written here with its exp(log(q)) threshold; nothing is
  consumed for p == 0);
* the charge loop zips winners, prices, second prices and outcomes: F = min(n, P - 1) slots are
  filled; every non-winner of every slot gets set_price, so after the loop every participant's
  logged price is price_{F-1} (0.0 when F = 0); a winner also logs its own second price, click and
  won = True;
* the counters of a record: src/Agent.py:96-118 over those log fields, each term rounded by
  tests/counter_reference.py fx.

Arrays are row-major as the fixtures: per (round, participant) [B][P], per (round, slot) [B][S].
"""
import math

import numpy as np

from counter_reference import (ALLOC_REGRET, BEST_EV, CTR_BIAS, CTR_SQERR, EST_REGRET, GROSS, N_LOGS, N_WON, NET,
                               OVERBID, PAID, UNDERBID, _div, _same_bits, fx)

FIRST_PRICE, SECOND_PRICE = 0, 1


def ranking(bids):
    """Participant slots by descending bid, ties to the lower slot."""
    return sorted(range(len(bids)), key=lambda s: -float(bids[s]))  # sorted() is stable


def allocate(mech, bids, n):
    """(winners, prices, second_prices) as the reference's allocate returns them (ragged)."""
    order = ranking(bids)
    srt = [float(bids[s]) for s in order]
    winners = order[:n]
    if mech == FIRST_PRICE:
        return winners, srt[:n], srt[1:n + 1]
    return winners, srt[1:n + 1], srt[1:n + 1]


def filled(n, P):
    """Slots the charge loop fills: zip stops at the second prices."""
    return min(n, P - 1)


def binomial1(p, u):
    """numpy Generator.binomial(1, p) from its next_double u (random_binomial_inversion, n = 1)."""
    if p == 0.0:
        return 0
    if p <= 0.5:
        return int(u > math.exp(math.log(1.0 - p)))
    q = 1.0 - p  # p > 0.5: 1 - binomial(1, 1 - p)
    return 1 - int(u > math.exp(math.log(1.0 - q)))


def consumed(n, P):
    """Doubles rng.binomial(1, CTRs[winners]) consumes."""
    return min(n, P)


def simulate(mech, fields, part, num_slots, u_slots, max_slots, N=None):
    """B multi-slot rounds. fields: value, bid, est_ctr, true_ctr, best_ev [B][P]; part [B][P];
    num_slots [B]; u_slots [B][>= min(max_slots, P)] (the k-th consumed double of a round in
    column k). Returns per slot [B][max_slots]: winner (-1 unfilled), price, second_price (NaN
    unfilled), outcome (0 unfilled); per round: log_price (NaN when F = 0), num_filled; per
    participant [B][P]: won_slot (-1: lost) and the log fields log_price_slot (0.0 when F = 0),
    log_second, log_outcome, log_won; counters [N][12] Python integers (units of 2^-36) and
    revenue, their PAID total."""
    part = np.asarray(part)
    B, P = part.shape
    if N is None:
        N = int(part.max()) + 1
    S = int(max_slots)
    col = {k: np.asarray(fields[k], np.float64) for k in ("value", "bid", "est_ctr", "true_ctr", "best_ev")}
    out = dict(winner=np.full((B, S), -1, np.int32), price=np.full((B, S), np.nan),
               second_price=np.full((B, S), np.nan), outcome=np.zeros((B, S), np.uint8),
               log_price=np.full(B, np.nan), num_filled=np.zeros(B, np.int32),
               won_slot=np.full((B, P), -1, np.int8), log_price_slot=np.zeros((B, P)),
               log_second=np.zeros((B, P)), log_outcome=np.zeros((B, P), bool), log_won=np.zeros((B, P), bool))
    tot = [[0] * 12 for _ in range(N)]
    for r in range(B):
        n = int(num_slots[r])
        assert 1 <= n <= S
        bids = col["bid"][r]
        winners, prices, seconds = allocate(mech, bids, n)
        outcomes = [binomial1(float(col["true_ctr"][r, w]), float(u_slots[r][k])) for k, w in enumerate(winners)]
        F = filled(n, P)
        assert F == min(len(winners), len(prices), len(seconds), len(outcomes))
        lp = prices[F - 1] if F > 0 else 0.0
        out["num_filled"][r] = F
        if F > 0:
            out["log_price"][r] = lp
        rank = {}
        for k in range(F):
            out["winner"][r, k] = winners[k]
            out["price"][r, k] = prices[k]
            out["second_price"][r, k] = seconds[k]
            out["outcome"][r, k] = outcomes[k]
            rank[winners[k]] = k
        for s in range(P):
            a = int(part[r, s])
            value, bid, est, tru, bev = (float(col[k][r, s]) for k in ("value", "bid", "est_ctr", "true_ctr",
                                                                      "best_ev"))
            tv = tru * value
            t = tot[a]
            k = rank.get(s, -1)
            out["won_slot"][r, s] = k
            out["log_price_slot"][r, s] = lp
            if k >= 0:
                out["log_second"][r, s] = seconds[k]
                out["log_outcome"][r, s] = bool(outcomes[k])
                out["log_won"][r, s] = True
                t[GROSS] += fx(value * float(outcomes[k]))
                t[PAID] += fx(prices[k])
                t[N_WON] += fx(1.0)
                t[OVERBID] += fx(lp - seconds[k])
                t[CTR_BIAS] += fx(1.0 if _same_bits(est, tru) else _div(est, tru))
            else:
                t[UNDERBID] += fx((lp - bid) * (1.0 if lp < tv else 0.0))
            t[ALLOC_REGRET] += fx(bev - tv)
            t[EST_REGRET] += fx(est * value - tv)
            d = tru - est
            t[CTR_SQERR] += fx(d * d)
            t[BEST_EV] += fx(bev)
            t[N_LOGS] += fx(1.0)
    for t in tot:
        t[NET] = t[GROSS] - t[PAID]
    out["counters"] = tot
    out["revenue"] = sum(t[PAID] for t in tot)
    return out


def allocate_padded(mech, bids, num_slots, max_slots):
    """allocate's three arrays for B rows of bids [B][P], padded to [B][max_slots] with -1 / NaN."""
    bids = np.asarray(bids, np.float64)
    B = bids.shape[0]
    w = np.full((B, max_slots), -1, np.int32)
    p = np.full((B, max_slots), np.nan)
    s = np.full((B, max_slots), np.nan)
    for r in range(B):
        ww, pp, ss = allocate(mech, bids[r], int(num_slots[r]))
        w[r, :len(ww)], p[r, :len(pp)], s[r, :len(ss)] = ww, pp, ss
    return w, p, s
