"""The twelve per-agent counters, stated plainly: no project code, no numpy arithmetic; the sums are
Python integers and the rounding is integer division (equal to round(Fraction(x) * 2**36), which
tests/test_counter_reference.py checks).

One log record per (auction, slot). Its terms are those of src/Agent.py:96-118 as the comment
block of oracle/ag_oracle.c simulate_range states them; each term x is a double and contributes

    round(Fraction(x) * 2**36), ties to even,   when abs(x) < 2**26,
    0                                           when it is larger or not finite,

to an unbounded Python integer (units of 2^-36). NET is GROSS - PAID. With P == 1 nothing is
charged: no record is won and the logged price is 0. CTR_BIAS of a won record is est_ctr / true_ctr,
and exactly 1 when the two are the same double bit for bit (include/auctiongym.h AG_FX_*).

to_limbs / from_limbs are the three 42-bit limbs of include/auctiongym.h: limbs 0 and 1 in
[0, 2^42), limb 2 signed (the normal form); from_limbs takes limbs in any form.
"""
import math
import struct

NAMES = ("net", "gross", "allocation_regret", "estimation_regret", "overbid_regret", "underbid_regret",
         "ctr_sqerr", "ctr_bias_sum", "best_ev_sum", "n_logs", "n_won", "paid")
(NET, GROSS, ALLOC_REGRET, EST_REGRET, OVERBID, UNDERBID, CTR_SQERR, CTR_BIAS, BEST_EV, N_LOGS, N_WON,
 PAID) = range(12)
FRAC_BITS, LIMB_BITS = 36, 42
_MASK = (1 << LIMB_BITS) - 1


def fx(x):
    """One term in units of 2^-36: nearest integer, ties to even; dropped (0) from 2^26 on."""
    x = float(x)
    if not math.isfinite(x) or abs(x) >= 2.0 ** 26:
        return 0
    n, d = x.as_integer_ratio()  # exact; d is a power of two
    q, r = divmod(n << FRAC_BITS, d)  # floor division: 0 <= r < d
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    return q  # == round(Fraction(x) * 2**36), which rounds half to even (test_fx_is_fraction_rounding)


def _same_bits(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def _div(a, b):
    """IEEE a / b (Python raises on b == 0)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def counters(outputs, part, P, N=None):
    """[N][12] Python integers in units of 2^-36 from the per-auction outputs: winner, price,
    second_price, outcome [B] and value, bid, est_ctr, true_ctr, best_ev [B][P]; part [B][P] names
    the agent of every slot. N defaults to the largest agent index seen, plus one."""
    part = part.tolist() if hasattr(part, "tolist") else [[int(a) for a in row] for row in part]
    if N is None:
        N = max(max(row) for row in part) + 1
    tot = [[0] * 12 for _ in range(N)]
    lst = lambda a: a.tolist() if hasattr(a, "tolist") else a  # noqa: E731  (plain Python floats and ints)
    col = [lst(outputs[k]) for k in ("value", "bid", "est_ctr", "true_ctr", "best_ev")]
    winner, outcome = lst(outputs["winner"]), lst(outputs["outcome"])
    prices, seconds = lst(outputs["price"]), lst(outputs["second_price"])
    charged = P >= 2
    for r, row in enumerate(part):
        w, oc = int(winner[r]), int(outcome[r])
        price = float(prices[r]) if charged else 0.0
        second = float(seconds[r]) if charged else 0.0
        for s, a in enumerate(row):
            value, bid, est, tru, bev = (float(c[r][s]) for c in col)
            won = charged and s == w
            tv = tru * value
            t = tot[a]
            if won:
                t[GROSS] += fx(value * float(oc))
                t[PAID] += fx(price)
                t[N_WON] += fx(1.0)
                t[OVERBID] += fx(price - second)
                t[CTR_BIAS] += fx(1.0 if _same_bits(est, tru) else _div(est, tru))
            else:
                t[UNDERBID] += fx((price - bid) * (1.0 if price < tv else 0.0))
            t[ALLOC_REGRET] += fx(bev - tv)
            t[EST_REGRET] += fx(est * value - tv)
            d = tru - est
            t[CTR_SQERR] += fx(d * d)
            t[BEST_EV] += fx(bev)
            t[N_LOGS] += fx(1.0)
    for t in tot:
        t[NET] = t[GROSS] - t[PAID]
    return tot


def to_limbs(v):
    """The normal form of an integer: limbs 0 and 1 in [0, 2^42), limb 2 signed."""
    v = int(v)
    return [v & _MASK, (v >> LIMB_BITS) & _MASK, v >> (2 * LIMB_BITS)]


def from_limbs(limbs):
    """limb0 + limb1 * 2^42 + limb2 * 2^84 for limbs in any form (e.g. summed over ranks)."""
    a, b, c = (int(x) for x in limbs)
    return a + (b << LIMB_BITS) + (c << (2 * LIMB_BITS))


def limbs_of(table):
    """counters()'s [N][12] integers as [N][12][3] normal-form limbs (nested lists)."""
    return [[to_limbs(v) for v in row] for row in table]
