"""The record collectors and the EmpiricalShadedBidder update at their edges.

k_shading_collect (csrc/ag_collect.hip) writes every record the learning bidders and the
EmpiricalShadedBidder update train on, k_lrts_collect (the same file) every sample the LR-TS
allocators train on. Both are pure functions of the arrays they are handed, so the reference here
is a plain numpy statement of include/auctiongym.h's description on host copies of exactly those
arrays (expected_records, expected_lrts_samples): every field of every record, bit for bit, the
count exact. The statements themselves are pinned without a GPU: the reference's own logs
(tests/golden/dr_update_kat.npz, empirical_update_kat.npz) are what expected_records derives from
the oracle's replay of the captures they were logged from.

Covered: P = 1 (nobody is charged: won == 0), batch tails around a wave and a workgroup, P = 8 and
the runtime-P kernel's P = 12, waves with no taker or one, one lane owning all of its wave's
records, a one-lane tail, the second grid-stride
pass (B = 2^20 + 37; 4096 workgroups of 256 lanes cover 2^20), a 64-bit order, the minimal store,
hand-made outputs in both layouts (the winner in the last slot, price above value, a won auction
without a click, bit 31 of the packed word), a store that overflows (guard tails past `capacity`
stay untouched, the count still counts, every update refuses), the agent buckets beyond one pass
of 256 agents (k_lrts_scan's carry, k_sh_hist), k_empirical_update on grids of 1 to 1024 buckets
with samples on the edges, exact ties, clamps and a masked launch, and the learning bidders' log
order beyond 40 bits (sort_records, csrc/ag_dr.hip).

empirical_plain is the documented rule in numpy; oracle.empirical_update (exact fixed-point sums
on a 2^-40 grid) equals it on every input set used here. Utilities that differ only below that
grid (N(0, 1) * 2^-45, say) are the oracle's stated limit and are kept out.
"""
import os
from collections import Counter

import numpy as np
import pytest

import test_gpu_trainer_branches as tb
from conftest import GOLDEN, load_capture, mech_code, pop_args
from test_gpu_parity import _empirical_engine, _fill_shading, _fill_store, _learner_store, _pop_engine
from test_gpu_shapes import _catalogue, _general_setup, _rounds, _upload

gpu_test = pytest.mark.gpu  # (per test: the reference tests below run without a GPU)

FIELDS = ("agent", "gamma", "utility", "ctr", "value", "propensity", "won", "order")
_DTYPES = {"agent": np.int32, "won": np.uint8, "order": np.uint64}
PER_FIELD = ("winner", "price", "second_price", "outcome", "item", "bid", "est_ctr", "true_ctr", "best_ev", "gamma",
             "propensity")
PACKED = ("winner_outcome",) + tuple(f for f in PER_FIELD if f not in ("winner", "outcome"))
BIG = (1 << 20) + 37  # one auction per lane: 4096 workgroups x 256 lanes = 2^20, then a second pass


# ---------------------------------------------------------------- 0. the plain references
def expected_records(part, out, bid_kind, values, P, first):
    """The records ag_shading_collect appends for auctions [first, first + B) (include/auctiongym.h
    ag_shading_samples), in (auction, slot) order. part [B][P]; out: row-major host arrays winner,
    outcome, price [B], item, gamma, est_ctr, propensity [B][P]; values [N][K]."""
    part = np.asarray(part)
    B = part.shape[0]
    assert part.shape == (B, P)
    i, s = np.nonzero(np.asarray(bid_kind)[part] != 0)  # every participation of a non-truthful bidder
    a = part[i, s]
    value = np.asarray(values, np.float64)[a, out["item"][i, s]]
    won = (out["winner"][i] == s) if P >= 2 else np.zeros(len(i), bool)  # P == 1: nobody is charged
    with np.errstate(invalid="ignore"):
        utility = np.where(won, value * out["outcome"][i].astype(np.float64) - out["price"][i], 0.0)
    order = (np.uint64(first) + i.astype(np.uint64)) * np.uint64(P) + s.astype(np.uint64)
    assert all(int(order[j]) == (first + int(i[j])) * P + int(s[j]) for j in (0, -1)[:len(i)])
    return dict(agent=a.astype(np.int32), gamma=out["gamma"][i, s], utility=utility, ctr=out["est_ctr"][i, s],
                value=value, propensity=out["propensity"][i, s], won=won.astype(np.uint8), order=order)


def expected_lrts_samples(ctx, part, out, alloc_kind, OE, P):
    """The samples ag_lrts_collect appends (ag_lrts_samples): for every auction whose winner is an
    LR-TS allocator, key = agent << 16 | item << 1 | outcome and x = float32(ctx[:OE]), 1.0f.
    Nothing at P == 1. -> (key uint32 [n], x float32 [n][OE + 1]) in auction order."""
    B = len(part)
    if P == 1:
        return np.zeros(0, np.uint32), np.zeros((0, OE + 1), np.float32)
    i = np.arange(B)
    w = out["winner"]
    a = part[i, w]
    take = np.asarray(alloc_kind)[a] == 1
    key = (a.astype(np.uint32) << 16) | (out["item"][i, w].astype(np.uint32) << 1) | (out["outcome"] != 0)
    x = np.concatenate([np.asarray(ctx)[:, :OE].astype(np.float32), np.ones((B, 1), np.float32)], axis=1)
    return key[take].astype(np.uint32), x[take]


def empirical_plain(gammas, utilities, detail=False):
    """EmpiricalShadedBidder.update as documented: buckets of 0.005 between the smallest and the
    largest gamma, the 1.96-sigma lower bound of the mean utility of every bucket with more than
    one sample, the last bucket with the largest bound, its midpoint clipped to [0, 1]."""
    g, u = np.asarray(gammas, np.float64), np.asarray(utilities, np.float64)
    lo, hi = float(g.min()), float(g.max())
    edges = np.linspace(lo, hi, int((hi - lo) // 0.005) + 1)
    bound = np.full(len(edges) - 1, -np.inf)
    for j in range(len(edges) - 1):
        inside = (edges[j] <= g) & (g < edges[j + 1])
        n = int(inside.sum())
        if n > 1:
            bound[j] = u[inside].mean() - 1.96 * (np.std(u[inside]) / np.sqrt(n))
    best = int(np.flatnonzero(bound == bound.max())[-1])
    assert np.isfinite(bound[best])
    gamma = float(np.clip((edges[best + 1] - edges[best]) / 2.0 + edges[best], 0.0, 1.0))
    return (gamma, edges, best) if detail else gamma


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _same(got, want):
    """Bit for bit; two NaNs (a field the bidder kind does not have) count as equal."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    eq = _bits(got) == _bits(want)
    if got.dtype == np.float64:
        eq |= np.isnan(got) & np.isnan(want)
    return bool(eq.all())


def _replay(oracle, name):
    d, meta, _ = load_capture(name)
    args = pop_args(d, meta)
    orc = oracle.simulate_pop(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"], **args)
    return d, meta, args, expected_records(d["part"], orc, args["bid_kind"], d["values"], meta["P"], 0)


DR_PREFIX = (661, 690, 697)  # records per agent of fp_dr_ts_r1024's 1024 rounds


def _check_dr_logs(recs, what):
    """Records of the fp_dr_ts_r1024 replay against the reference's logs (dr_update_kat.npz a{i}_*:
    1350 records per agent, the capture's rounds are their prefix)."""
    k = np.load(os.path.join(GOLDEN, "dr_update_kat.npz"))
    worst = 0.0
    for a, n in enumerate(DR_PREFIX):
        sel = recs["agent"] == a
        assert int(sel.sum()) == n, (what, a)
        assert np.all(np.diff(recs["order"][sel].astype(np.int64)) > 0)  # round order
        for f, name, dt in (("gamma", "gamma", np.float64), ("ctr", "est_ctr", np.float64), ("value", "value", np.float64),
                            ("won", "won", np.uint8), ("utility", "util", np.float64)):
            assert _same(recs[f][sel], k[f"a{a}_{name}"][:n].astype(dt)), (what, a, f)
        want = k[f"a{a}_propensity"][:n]
        worst = max(worst, float(np.max(np.abs(recs["propensity"][sel] - want) / np.abs(want))))
    print(f"{what}: propensity vs the reference's logs, worst relative difference {worst:.3g}")
    assert worst <= 1e-15


def _check_empirical_logs(recs, what):
    """Records of the fp_empirical_r2048 replay against empirical_update_kat.npz c0_it0, full length."""
    k = np.load(os.path.join(GOLDEN, "empirical_update_kat.npz"))
    for a in range(6):
        sel = recs["agent"] == a
        assert _same(recs["gamma"][sel], k[f"c0_it0_a{a}_gammas"]), (what, a)
        assert _same(recs["utility"][sel], k[f"c0_it0_a{a}_util"]), (what, a)
    return k


def test_record_reference_matches_reference_logs(oracle):
    """expected_records on the oracle's replay of fp_dr_ts_r1024 and fp_empirical_r2048 gives, agent
    by agent in round order, the reference's own logs: gamma, est_ctr, value, won and utility bit for
    bit, the propensity within 1e-15 relative (a few ulps of libm's exp and log between the two
    hosts; the worst is printed: 2.8e-16 .. 3.4e-16 measured)."""
    _check_dr_logs(_replay(oracle, "fp_dr_ts_r1024")[3], "oracle replay")
    _check_empirical_logs(_replay(oracle, "fp_empirical_r2048")[3], "oracle replay")


# ---------------------------------------------------------------- empirical input sets (section 5)
def _grid(lo, hi):
    return np.linspace(lo, hi, int((hi - lo) // 0.005) + 1)


def _empirical_cases():
    """name -> (gammas, utilities, winning bucket or None)."""
    g = np.random.default_rng(77)
    u = lambda n, s=0.3: g.normal(0.05, s, n)  # noqa: E731
    c = {}
    x = g.uniform(0, 1, 6000)
    c["uniform_199"] = (x, u(6000), None)
    e = np.linspace(0.1, 0.9, 161)
    c["on_every_edge"] = (np.repeat(e, 7), u(161 * 7), None)
    e = np.linspace(0.25, 0.75, 100)
    four = np.array([0.25, -0.5, 0.75, 0.0])
    ut = np.concatenate([g.permutation(four) for _ in range(99)] + [[0.0]])
    c["ties_all"] = (np.concatenate([np.repeat(e[:99], 4), [0.75]]), ut, 98)
    low = np.repeat(~np.isin(np.arange(99), (10, 57)), 4)
    ut2 = ut.copy()
    ut2[:396][low] -= 0.125
    c["ties_10_57"] = (c["ties_all"][0], ut2, 57)
    e = _grid(0.2, 0.8)
    c["below_edges"] = (np.concatenate([[0.2, 0.2, 0.8], np.repeat(np.nextafter(e[1:], 0.0), 3)]), u(3 + 3 * (len(e) - 1)),
                        None)
    x = g.uniform(0.3, 0.7, 3000)
    c["constant_utility"] = (x, np.full(3000, 0.125), len(_grid(x.min(), x.max())) - 2)
    c["zero_utility"] = (g.uniform(0.3, 0.7, 3000), np.zeros(3000), None)
    c["negative"] = (g.uniform(0.3, 0.7, 3000), -1000.0 + 1000.0 * g.random(3000), None)
    c["clamp_0"] = (g.uniform(-0.2, -0.15, 1000), u(1000), None)
    c["clamp_1"] = (g.uniform(1.3, 1.35, 1000), u(1000), None)
    c["at_max"] = (np.concatenate([g.uniform(0.4, 0.6, 2000), np.full(500, 0.62)]), u(2500), None)
    c["n3_one_bucket"] = (np.array([0.5, 0.502, 0.507]), np.array([0.25, -0.125, 3.0]), 0)
    x = g.uniform(0.5, 0.512, 200000)
    x[:2] = 0.5, 0.512
    c["n200k_two_buckets"] = (x, u(200000), None)
    x = g.uniform(0, 5.1249, 20000)
    x[:2] = 0.0, 5.1249
    c["buckets_1024"] = (x, u(20000), None)
    return c


_BUCKETS = {"uniform_199": 199, "on_every_edge": 160, "ties_all": 99, "n3_one_bucket": 1, "n200k_two_buckets": 2,
            "buckets_1024": 1024}


def test_empirical_oracle_matches_plain_statement(oracle):
    """oracle.empirical_update == empirical_plain exactly on every input set of
    test_empirical_update_edges, and the sets are what they claim: the bucket counts, samples on the
    edges of the grid the update builds, ties that pick the last maximum, samples one ulp below an
    edge, clamps on both sides. (Utilities that differ only below the oracle's 2^-40 fixed-point grid
    are its stated limit: none here.)"""
    for name, (gm, ut, best) in _empirical_cases().items():
        want, edges, b = empirical_plain(gm, ut, detail=True)
        assert oracle.empirical_update(gm, ut) == want, name
        if name in _BUCKETS:
            assert len(edges) - 1 == _BUCKETS[name], (name, len(edges) - 1)
        if best is not None:
            assert b == best, (name, b)
        if name in ("on_every_edge", "ties_all", "ties_10_57"):
            assert np.isin(gm, edges).all(), name
        if name == "below_edges":
            assert np.isin(np.nextafter(gm[3:], 1.0), edges[1:]).all() and not np.isin(gm[3:], edges).any()
        if name == "at_max":
            assert (gm == edges[-1]).sum() == 500
        if name.startswith("clamp"):
            assert want == float(name[-1]) and not 0.0 <= gm.mean() <= 1.0
        if name == "negative":
            assert ut.max() < 0 and ut.min() >= -1000


# ---------------------------------------------------------------- GPU helpers
def _host_out(out):
    """Device outputs -> row-major host arrays; winner and outcome from the packed word if that is what there is."""
    o = {k: v.cpu().numpy() for k, v in out.items()}
    if "winner_outcome" in o:
        wo = o.pop("winner_outcome").view(np.uint32)
        o["winner"], o["outcome"] = (wo & 0x7fffffff).astype(np.int32), (wo >> 31).astype(np.uint8)
    for k in ("item", "gamma", "est_ctr", "propensity"):
        if k in o:
            o[k] = np.ascontiguousarray(o[k].T)
    return o


def _records(st, n=None):
    n = int(st["count"].item()) if n is None else n
    r = {f: st[f][:n].cpu().numpy() for f in FIELDS if f in st}
    if "order" in r:
        r["order"] = r["order"].view(np.uint64)
    return r


def _assert_records(got, want, what):
    """Every field of every record, matched by order (unique per record), bit for bit."""
    assert len(got["order"]) == len(want["order"]), (what, len(got["order"]), len(want["order"]))
    idx = np.argsort(got["order"], kind="stable")
    for f in FIELDS:
        assert _same(got[f][idx], np.asarray(want[f]).astype(_DTYPES.get(f, np.float64))), (what, f)


def _collect(eng, inp, B, fields, first=0, learning=True, capacity=None):
    """simulate B auctions into `fields`, collect them into a fresh store -> (store, host outputs)."""
    import torch
    out = eng.alloc_outputs(B, fields)
    eng.simulate(inp, out)
    st = eng.new_shading_samples(capacity or eng.P * B, learning=learning)
    eng.shading_collect(inp, out, st, first_auction=first)
    torch.cuda.synchronize()
    return st, _host_out(out)


def _guarded(shape, dtype, sentinel, guard, device):
    """One flat tensor of prod(shape) + guard elements, all `sentinel`: the leading view of `shape`
    (a store field whose capacity is the view's length) and the guard tail."""
    import torch
    n = int(np.prod(shape))
    flat = torch.full((n + guard,), sentinel, dtype=dtype, device=device)
    return flat[:n].view(*shape), flat[n:]


# ---------------------------------------------------------------- 1. the reference's logs
@gpu_test
@pytest.mark.parametrize("name", ["fp_dr_ts_r1024", "fp_empirical_r2048"])
def test_shading_collect_reproduces_reference_logs(gpu, oracle, name):
    """The capture replayed on the GPU in two flushes (first_auction 0 and B / 2) into one learning
    store, from per-field outputs and from the winner | outcome word: every field equals
    expected_records on the oracle's outputs and the reference's own logs; ag_shading_counts gives the
    logs' lengths; for the EmpiricalShadedBidder capture ag_empirical_update from that store gives the
    reference's next prev_gamma."""
    import torch
    d, meta, args, want = _replay(oracle, name)
    B, P = len(d["u"]), meta["P"]
    for fields in (PER_FIELD, PACKED):
        eng, _ = _pop_engine(meta, d, gpu)
        inp = _upload(eng, d["ctx"], d["part"], d["u"], gamma_raw=d["gamma_raw"], ts_noise=d.get("ts_noise"))
        st = eng.new_shading_samples(P * B, learning=True)
        for lo, hi in ((0, B // 2), (B // 2, B)):
            bi = {k: (v[..., lo:hi] if k != "ts_noise" else v[:, lo // 64:hi // 64]).contiguous() for k, v in inp.items()}
            bo = eng.alloc_outputs(hi - lo, fields)
            eng.simulate(bi, bo)
            eng.shading_collect(bi, bo, st, first_auction=lo)
        torch.cuda.synchronize()
        got = _records(st)
        _assert_records(got, want, (name, fields[0]))
        idx = np.lexsort((got["order"], got["agent"]))  # (agent, order): the logs' order
        got = {f: v[idx] for f, v in got.items()}
        counts = eng.shading_counts(st)
        if name == "fp_dr_ts_r1024":
            _check_dr_logs(got, f"GPU {fields[0]}")
            assert tuple(counts) == DR_PREFIX
        else:
            k = _check_empirical_logs(got, f"GPU {fields[0]}")
            assert list(counts) == [len(k[f"c0_it0_a{a}_gammas"]) for a in range(6)]
            assert list(eng.empirical_update(st)) == [float(k[f"c0_it0_a{a}_pg1"]) for a in range(6)]
        eng.close()


# ---------------------------------------------------------------- 2. the shading collector's edges
@gpu_test
@pytest.mark.parametrize("P,B", [(1, 257), (2, 1), (2, 63), (2, 64), (2, 65), (2, 257), (8, 549), (12, 549)])
def test_shading_collect_shapes(gpu, P, B):
    """Every bidder kind and learner state (_general_setup's "all" population of 20 agents) at P = 1
    (every record: won == 0, utility == 0.0), P = 2 around a wave and a workgroup, P = 8 (streamed
    slots) and P = 12 (the runtime-P kernel), both output layouts: every record equals
    expected_records on the outputs the collector was handed."""
    eng, (ctx, part, u, more), _, pop = _general_setup(4100 + 16 * P + B, 20, P, 12, 5, 4, 0 if P == 1 else B % 2, "all", B=B)
    if B == 1:
        part[0] = (2, 3)  # two EmpiricalShadedBidders
    inp = _upload(eng, ctx, part, u, **more)
    for fields in (PER_FIELD, PACKED):
        st, out = _collect(eng, inp, B, fields)
        want = expected_records(part, out, pop["bk"], pop["values"], P, 0)
        assert len(want["order"]) == int((pop["bk"][part] != 0).sum()) > 0
        _assert_records(_records(st), want, (P, B, fields[0]))
        if P == 1:
            got = _records(st)
            assert not got["won"].any() and not _bits(got["utility"]).any()
        else:
            assert want["won"].any() and (want["utility"] != 0).any()
    eng.close()


def _shading_engine(N, P, bk, seed, mech=0):
    """Oracle allocators, bidder kinds bk (Gaussian shading from gamma_raw), the suite's catalogue recipe."""
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(seed)
    items, values = _catalogue(g, N, 12, 5)
    pg, gs = 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N)
    eng = AuctionEngine(N, P, 12, 5, 4, mech, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), bk, pg, gs)
    eng.load_catalog(items, values)
    return eng, g, values, pg, gs


@gpu_test
def test_shading_collect_sparse_ballots(gpu):
    """64 agents, P = 2, agent 0 the only shading bidder: most waves of 64 auctions have nobody to
    record in a slot (the ballot is empty and the wave skips it) or a single taker."""
    N, P, B = 64, 2, 3001
    bk = np.zeros(N, np.int32)
    bk[0] = 1
    eng, g, values, pg, gs = _shading_engine(N, P, bk, 61)
    ctx, part, u = _rounds(g, N, P, 5, B)
    takers = np.add.reduceat((part == 0).astype(np.int64), np.arange(0, B, 64), axis=0)  # per (wave, slot)
    assert (takers == 0).sum() > 10 and (takers == 1).sum() > 10 and (takers > 1).any()
    inp = _upload(eng, ctx, part, u, gamma_raw=g.normal(pg[part], gs[part]))
    for fields in (PER_FIELD, PACKED):
        st, out = _collect(eng, inp, B, fields)
        want = expected_records(part, out, bk, values, P, 0)
        assert len(want["order"]) == int(takers.sum())
        _assert_records(_records(st), want, fields[0])
    eng.close()


@gpu_test
def test_shading_collect_second_grid_stride_pass(gpu):
    """B = 2^20 + 37 at P = 2: the launch is capped at 4096 workgroups of 256 lanes, so the last 37
    auctions are a second pass of the grid-stride loop. EmpiricalShadedBidders on a quarter of the 8
    agents; inputs drawn on the device, simulated on the device; every one of the ~524k records
    checked, and ag_shading_counts (k_sh_hist's own grid-stride loop stays below its cap here)."""
    N, P, B = 8, 2, BIG
    bk = np.array([1, 1, 0, 0, 0, 0, 0, 0], np.int32)
    eng, _, values, _, _ = _shading_engine(N, P, bk, 62)
    inp = eng.alloc_inputs(B)
    eng.generate(21, 0, inp)
    eng.generate_noise(21, 0, inp)
    st, out = _collect(eng, inp, B, None)
    part = np.ascontiguousarray(inp["part"].cpu().numpy().T)
    want = expected_records(part, out, bk, values, P, 0)
    assert (want["order"] >= np.uint64((1 << 20) * P)).any()  # the second pass has records
    got = _records(st)
    _assert_records(got, want, "second pass")
    assert np.array_equal(eng.shading_counts(st), np.bincount(want["agent"], minlength=N))
    eng.close()


@gpu_test
def test_shading_collect_order_is_64_bit_and_minimal_store(gpu):
    """first_auction = 2^33 + 5: order == (first + i) * P + s exactly (beyond 32 bits). And a
    learning=False store of the same outputs holds the same (agent, gamma, utility) multiset."""
    P, B, first = 2, 257, (1 << 33) + 5
    eng, (ctx, part, u, more), _, pop = _general_setup(4321, 20, P, 12, 5, 4, 0, "all", B=B)
    inp = _upload(eng, ctx, part, u, **more)
    st, out = _collect(eng, inp, B, PER_FIELD, first=first)
    want = expected_records(part, out, pop["bk"], pop["values"], P, first)
    assert int(want["order"][0]) >= first * P > 1 << 34
    _assert_records(_records(st), want, "order")
    small, out2 = _collect(eng, inp, B, PER_FIELD, first=first, learning=False)
    assert set(small) == {"agent", "gamma", "utility", "count"}
    got = _records(small)
    rows = lambda r: sorted(zip(r["agent"].tolist(), _bits(r["gamma"]).tolist(), _bits(r["utility"]).tolist()))  # noqa: E731
    assert rows(got) == rows(want) and len(got["agent"]) == len(want["agent"])
    eng.close()


@gpu_test
def test_shading_collect_hand_made_outputs(gpu):
    """No simulate: outputs written by hand, in both layouts (bit 31 of the packed word is the click).
    The winner in the last slot, a price above the value (negative utility), a won auction without a
    click (utility = -price), and 70 random rows."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    N, P, K, B = 5, 3, 12, 70
    g = np.random.default_rng(63)
    bk = np.array([1, 4, 0, 3, 2], np.int32)
    items, values = _catalogue(g, N, K, 5)
    eng = AuctionEngine(N, P, K, 5, 4, 0, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), bk, np.ones(N), np.full(N, 0.05))
    eng.load_catalog(items, values)
    _, part, _ = _rounds(g, N, P, 5, B)
    out = dict(winner=g.integers(0, P, B).astype(np.int32), outcome=(g.random(B) < 0.5).astype(np.uint8),
               price=g.uniform(0.1, 2.5, B), item=g.integers(0, K, (B, P)).astype(np.int32),
               gamma=g.uniform(0, 1.2, (B, P)), est_ctr=g.random((B, P)), propensity=g.uniform(0.1, 9, (B, P)))
    part[0], out["winner"][0], out["outcome"][0], out["price"][0] = (2, 4, 0), P - 1, 1, 50.0  # last slot, price > value
    part[1], out["winner"][1], out["outcome"][1] = (3, 2, 1), 0, 0                              # won, no click
    want = expected_records(part, out, bk, values, P, 7)
    first_row = want["order"] < np.uint64(8 * P)
    assert list(want["won"][first_row]) == [0, 1] and want["utility"][first_row][1] < -40
    second = (want["order"] >= np.uint64(8 * P)) & (want["order"] < np.uint64(9 * P))
    assert list(want["won"][second]) == [1, 0] and want["utility"][second][0] == -out["price"][1]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    inp = {"part": up(part.T), "u": up(np.zeros(B))}
    dev = {k: up(v.T if v.ndim == 2 else v) for k, v in out.items()}
    word = (out["winner"].astype(np.uint32) | (out["outcome"].astype(np.uint32) << 31)).view(np.int32)
    assert (word < 0).any()
    packed = {k: v for k, v in dev.items() if k not in ("winner", "outcome")}
    packed["winner_outcome"] = up(word)
    for name, o in (("fields", dev), ("packed", packed)):
        st = eng.new_shading_samples(P * B, learning=True)
        eng.shading_collect(inp, o, st, first_auction=7)
        torch.cuda.synchronize()
        _assert_records(_records(st), want, name)
    eng.close()


@gpu_test
def test_shading_collect_one_lane_owns_every_record_of_its_wave(gpu):
    """Hand-made outputs, no simulate: P = 4, B = 130 (two full waves and a 2-lane tail). Only the
    auction at lane 1 of each wave (1, 65, 129) has non-truthful bidders, and it has them in all four
    slots: one lane owns its wave's four records and its neighbours none, the case a per-lane prefix
    sum can get wrong. Both output layouts, first_auction = 11."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    N, P, K, B = 8, 4, 12, 130
    g = np.random.default_rng(64)
    bk = np.array([1, 4, 3, 2, 0, 0, 0, 0], np.int32)
    items, values = _catalogue(g, N, K, 5)
    eng = AuctionEngine(N, P, K, 5, 4, 0, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), bk, np.ones(N), np.full(N, 0.05))
    eng.load_catalog(items, values)
    owners = np.array([1, 65, 129])
    part = np.tile(np.arange(4, 8, dtype=np.int32), (B, 1))
    part[owners] = [(0, 1, 2, 3), (3, 2, 1, 0), (2, 0, 3, 1)]
    out = dict(winner=g.integers(0, P, B).astype(np.int32), outcome=(g.random(B) < 0.5).astype(np.uint8),
               price=g.uniform(0.1, 2.5, B), item=g.integers(0, K, (B, P)).astype(np.int32),
               gamma=g.uniform(0, 1.2, (B, P)), est_ctr=g.random((B, P)), propensity=g.uniform(0.1, 9, (B, P)))
    out["outcome"][owners] = 1, 0, 1
    want = expected_records(part, out, bk, values, P, 11)
    assert len(want["order"]) == 4 * len(owners) and int(want["won"].sum()) == len(owners)
    assert sorted(set(int(o) // P - 11 for o in want["order"])) == list(owners)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    inp = {"part": up(part.T), "u": up(np.zeros(B))}
    dev = {k: up(v.T if v.ndim == 2 else v) for k, v in out.items()}
    word = (out["winner"].astype(np.uint32) | (out["outcome"].astype(np.uint32) << 31)).view(np.int32)
    packed = {k: v for k, v in dev.items() if k not in ("winner", "outcome")}
    packed["winner_outcome"] = up(word)
    for name, o in (("fields", dev), ("packed", packed)):
        st = eng.new_shading_samples(P * B, learning=True)
        eng.shading_collect(inp, o, st, first_auction=11)
        torch.cuda.synchronize()
        assert int(st["count"].item()) == 4 * len(owners), name
        _assert_records(_records(st), want, name)
    eng.close()


@gpu_test
def test_shading_collect_overflow_stays_inside_the_store(gpu):
    """A store 37 records too small, every field with a guard tail of sentinels right behind
    `capacity`: count still counts every record, the store holds `capacity` distinct records of the
    expected set, no guard element is touched, and ag_empirical_update, ag_shading_counts and
    ag_bidder_update refuse the store ("overflowed"). The designed behaviour of a full store."""
    import torch
    P, B, G = 2, 549, 256
    eng, (ctx, part, u, more), _, pop = _general_setup(4400, 20, P, 12, 5, 4, 0, "all", B=B)
    inp = _upload(eng, ctx, part, u, **more)
    out = eng.alloc_outputs(B, PER_FIELD)
    eng.simulate(inp, out)
    want = expected_records(part, _host_out(out), pop["bk"], pop["values"], P, 0)
    R = len(want["order"])
    C = R - 37
    assert C > 256
    sent = {"agent": -7, "won": 0xAB, "order": -99}
    dt = {"agent": torch.int32, "won": torch.uint8, "order": torch.int64}
    st, guards = {"count": torch.zeros(1, dtype=torch.int64, device=eng.device)}, {}
    for f in FIELDS:
        st[f], guards[f] = _guarded((C,), dt.get(f, torch.float64), sent.get(f, -12345.678), G, eng.device)
    eng.shading_collect(inp, out, st)
    torch.cuda.synchronize()
    assert int(st["count"].item()) == R
    for f in FIELDS:
        assert bool((guards[f] == sent.get(f, -12345.678)).all()), f
    got = _records(st, C)
    assert len(np.unique(got["order"])) == C and np.isin(got["order"], want["order"]).all()
    kept = np.isin(want["order"], got["order"])
    _assert_records(got, {f: v[kept] for f, v in want.items()}, "the records that fitted")
    for call in (lambda: eng.empirical_update(st), lambda: eng.shading_counts(st),
                 lambda: eng.bidder_update(st, None, np.zeros(20, np.int64), 0)):
        with pytest.raises(ValueError, match="overflow"):
            call()
    eng.close()


@gpu_test
def test_shading_collect_without_shading_bidders(gpu):
    """A TruthfulBidder-only population: the call succeeds and appends nothing."""
    import torch
    eng, (ctx, part, u, more), _, _ = _general_setup(4500, 8, 2, 12, 5, 4, 1, "ts", B=65)
    inp = _upload(eng, ctx, part, u, **more)
    out = eng.alloc_outputs(65)
    eng.simulate(inp, out)
    st = eng.new_shading_samples(16, learning=True)
    eng.shading_collect(inp, out, st)
    torch.cuda.synchronize()
    assert int(st["count"].item()) == 0
    eng.close()


# ---------------------------------------------------------------- 3. the LR-TS collector's edges
def _lrts_rows(key, x):
    """(key, x-row) records as sorted rows of uint32 words: a multiset."""
    rows = np.concatenate([np.asarray(key).view(np.uint32)[:, None], np.ascontiguousarray(x, np.float32).view(np.uint32)],
                          axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def _lrts_store_rows(st, n=None):
    n = int(st["count"].item()) if n is None else n
    return _lrts_rows(st["key"][:n].cpu().numpy(), st["x"][:, :n].cpu().numpy().T)


def _lrts_population(N, P, ak, seed, mech=1):
    """LR-TS (ak == 1) and Oracle allocators, TruthfulBidders, MAP item choice (no Thompson noise to draw)."""
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(seed)
    items, values = _catalogue(g, N, 12, 5)
    eng = AuctionEngine(N, P, 12, 5, 4, mech, 1.0)
    eng.set_agent_params(ak, np.zeros(N, np.int32))
    eng.load_catalog(items, values)
    eng.load_lrts(g.normal(0, 1, (N, 12, 5)).astype(np.float32), np.ones((N, 12, 5), np.float32), thompson_sampling=False)
    return eng, g


@gpu_test
def test_lrts_collect_p1_collects_nothing(gpu):
    """P == 1: nobody is charged, no sample is won."""
    import torch
    eng, g = _lrts_population(4, 1, np.ones(4, np.int32), 71, mech=0)
    ctx, part, u = _rounds(g, 4, 1, 5, 257)
    inp = _upload(eng, ctx, part, u)
    out = eng.alloc_outputs(257)
    eng.simulate(inp, out)
    st = eng.new_lrts_samples(257)
    eng.lrts_collect(inp, out, st)
    torch.cuda.synchronize()
    assert int(st["count"].item()) == 0
    assert len(expected_lrts_samples(ctx, part, _host_out(out), np.ones(4, np.int32), 4, 1)[0]) == 0
    eng.close()


@gpu_test
def test_lrts_collect_one_wave_and_one_lane(gpu):
    """B = 65 at P = 2, every agent an LR-TS allocator: one full wave and a 1-lane tail, every
    auction a sample."""
    import torch
    ak = np.ones(4, np.int32)
    eng, g = _lrts_population(4, 2, ak, 73)
    ctx, part, u = _rounds(g, 4, 2, 5, 65)
    inp = _upload(eng, ctx, part, u)
    out = eng.alloc_outputs(65)
    eng.simulate(inp, out)
    st = eng.new_lrts_samples(65)
    eng.lrts_collect(inp, out, st)
    torch.cuda.synchronize()
    key, x = expected_lrts_samples(ctx, part, _host_out(out), ak, 4, 2)
    assert int(st["count"].item()) == len(key) == 65
    assert np.array_equal(_lrts_store_rows(st), _lrts_rows(key, x))
    eng.close()


@gpu_test
def test_lrts_collect_second_grid_stride_pass(gpu):
    """B = 2^20 + 37, LR-TS and Oracle allocators alternating among 8 agents: the (key, x) multiset
    equals expected_lrts_samples on the device-made inputs, the second pass's 37 auctions included."""
    import torch
    N, P, B = 8, 2, BIG
    ak = np.array([i % 2 for i in range(N)], np.int32)
    eng, _ = _lrts_population(N, P, ak, 72)
    inp = eng.alloc_inputs(B)
    assert "ts_noise" not in inp
    eng.generate(23, 0, inp)
    out = eng.alloc_outputs(B)
    eng.simulate(inp, out)
    st = eng.new_lrts_samples(B)
    eng.lrts_collect(inp, out, st)
    torch.cuda.synchronize()
    ctx, part = inp["ctx"].cpu().numpy().T, np.ascontiguousarray(inp["part"].cpu().numpy().T)
    o = _host_out(out)
    key, x = expected_lrts_samples(ctx, part, o, ak, 4, P)
    assert int(st["count"].item()) == len(key) > B // 4
    assert (ak[part[np.arange(B), o["winner"]]][1 << 20:] == 1).any()  # the second pass wins samples
    assert np.array_equal(_lrts_store_rows(st), _lrts_rows(key, x))
    eng.close()


@gpu_test
def test_lrts_collect_one_agent_two_flushes_both_layouts_and_overflow(gpu):
    """One LR-TS allocator among 64 agents (waves with an empty ballot, waves with one taker). Two
    flushes appended to one store, the first from per-field outputs, the second from the
    winner | outcome word. Then the same into a store too small, with guard tails behind key and
    behind the [OE + 1][capacity] block of x: the count is exact, the store holds a sub-multiset of
    the expected samples (a write past a row's capacity would land in the next row), the guards are
    intact and ag_lrts_update refuses it."""
    import torch
    N, P, B, G = 64, 2, 6002, 256
    ak = np.zeros(N, np.int32)
    ak[5] = 1
    eng, g = _lrts_population(N, P, ak, 73)
    ctx, part, u = _rounds(g, N, P, 5, B)
    inp = _upload(eng, ctx, part, u)
    halves = []
    for lo, hi, fields in ((0, B // 2, PER_FIELD[:9]), (B // 2, B, ("winner_outcome",) + PER_FIELD[1:3] + PER_FIELD[4:9])):
        bi = {k: v[..., lo:hi].contiguous() for k, v in inp.items()}
        bo = eng.alloc_outputs(hi - lo, fields)
        eng.simulate(bi, bo)
        halves.append((bi, bo, expected_lrts_samples(ctx[lo:hi], part[lo:hi], _host_out(bo), ak, 4, P)))
    key = np.concatenate([h[2][0] for h in halves])
    x = np.concatenate([h[2][1] for h in halves])
    R = len(key)
    assert 50 < R < B // 16 and set(key >> 16) == {5}
    st = eng.new_lrts_samples(R)
    for bi, bo, _ in halves:
        eng.lrts_collect(bi, bo, st)
    torch.cuda.synchronize()
    assert int(st["count"].item()) == R
    assert np.array_equal(_lrts_store_rows(st), _lrts_rows(key, x))
    # overflow
    C = R - 37
    kview, kguard = _guarded((C,), torch.int32, -7, G, eng.device)
    xview, xguard = _guarded((5, C), torch.float32, -12345.5, G, eng.device)
    small = {"key": kview, "x": xview, "count": torch.zeros(1, dtype=torch.int64, device=eng.device)}
    for bi, bo, _ in halves:
        eng.lrts_collect(bi, bo, small)
    torch.cuda.synchronize()
    assert int(small["count"].item()) == R
    assert bool((kguard == -7).all()) and bool((xguard == -12345.5).all())
    rows = lambda r: Counter(map(bytes, r))  # noqa: E731
    got, all_rows = rows(_lrts_store_rows(small, C)), rows(_lrts_rows(key, x))
    assert sum(got.values()) == C and not got - all_rows
    with pytest.raises(ValueError, match="overflow"):
        eng.lrts_update(small)
    eng.close()


# ---------------------------------------------------------------- 4. more than 256 agents
@gpu_test
def test_agent_buckets_beyond_one_pass_of_256(gpu, oracle):
    """300 agents (K = 3, OE + 1 = 2): k_lrts_scan scans the per-agent counts 256 at a time and
    carries the running sum into the second pass. Agents 0, 255, 256 and 299 train on ~40 samples each
    and equal oracle.lrts_update (epochs, m, q, prev_m); agents with one sample or none keep what was
    loaded, bit for bit. And ag_shading_counts (k_sh_hist) of a 300-agent store == np.bincount."""
    from auctiongym_amd.engine import AuctionEngine
    N, K, Do = 300, 3, 2
    g = np.random.default_rng(81)
    eng = AuctionEngine(N, 2, K, 2, Do - 1, 1, 1.0)
    eng.set_agent_params(np.ones(N, np.int32), np.zeros(N, np.int32))
    m0 = g.normal(0, 1, (N, K, Do)).astype(np.float32)
    q0 = (1 + g.random((N, K, Do))).astype(np.float32)
    pm0 = (m0 + 0.25).astype(np.float32)
    eng.load_lrts(m0, q0, pm0)

    def samples(n):
        X = np.concatenate([g.normal(0, 1, (n, Do - 1)), np.ones((n, 1))], axis=1)
        return X, g.integers(0, K, n), g.random(n) < 0.4
    trained = {0: samples(40), 255: samples(37), 256: samples(43), 299: samples(40)}
    single = {a: samples(1) for a in (1, 100, 254, 257, 298)}
    st = _fill_store(eng, {**trained, **single})
    ep = eng.lrts_update(st)
    m, q, pm = eng.lrts_state()
    for a, (X, A, y) in trained.items():
        om, opm, oq, oep, _ = oracle.lrts_update(X, A, y, m0[a], pm0[a], q0[a])
        assert ep[a] == oep > 0, a
        assert np.array_equal(m[a], om) and np.array_equal(q[a], oq) and np.array_equal(pm[a], opm), a
    rest = np.setdiff1d(np.arange(N), list(trained))
    assert not ep[rest].any()
    for got, was in ((m, m0), (q, q0), (pm, pm0)):
        assert np.array_equal(got[rest].view(np.uint32), was[rest].view(np.uint32))
    eng.close()
    eng = AuctionEngine(N, 2, K, 2, Do - 1, 0, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), np.ones(N, np.int32), np.full(N, 0.9), np.full(N, 0.05))
    n = g.integers(0, 9, N)
    n[[0, 255, 256, 299]] = 11, 3, 5, 7
    n[[2, 258]] = 0
    sh = _fill_shading(eng, {a: (g.random(n[a]), g.random(n[a])) for a in range(N)})
    assert np.array_equal(eng.shading_counts(sh), n)
    eng.close()


# ---------------------------------------------------------------- 5. the empirical update's edges
def _edge_population(extra=0):
    """The edge input sets as EmpiricalShadedBidders at the even agents, DoublyRobustBidders with
    records of their own (in the same store, interleaved) at the odd ones; `extra` further
    EmpiricalShadedBidders without a record at the end."""
    from auctiongym_amd.engine import AuctionEngine
    cases = _empirical_cases()
    N = 2 * len(cases) + extra
    bk = np.array([1 if a % 2 == 0 or a >= 2 * len(cases) else 4 for a in range(N)], np.int32)
    pg0 = 0.5 + np.arange(N) / 256.0
    eng = AuctionEngine(N, 2, 12, 5, 4, 0, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), bk, pg0, np.full(N, 0.05))
    g = np.random.default_rng(91)
    eng.load_catalog(g.normal(size=(N, 12, 6)), g.random((N, 12)))
    per = {}
    for j, (gm, ut, _) in enumerate(cases.values()):
        per[2 * j] = (gm, ut)
        per[2 * j + 1] = (g.uniform(0, 1, 500), g.normal(0.5, 1, 500))  # would win other buckets
    return eng, cases, per, pg0


@gpu_test
def test_empirical_update_edges(gpu, oracle):
    """Every edge input set in one launch (one workgroup per agent), the other agents' records
    shuffled into the same store: prev_gamma == oracle.empirical_update exactly (== empirical_plain,
    test_empirical_oracle_matches_plain_statement); the DoublyRobustBidders' prev_gamma untouched."""
    eng, cases, per, pg0 = _edge_population()
    pg = eng.empirical_update(_fill_shading(eng, per, seed=5))
    for j, (name, (gm, ut, _)) in enumerate(cases.items()):
        assert pg[2 * j] == oracle.empirical_update(gm, ut), name
        assert pg[2 * j + 1] == pg0[2 * j + 1], name
    eng.close()


@gpu_test
def test_empirical_update_refuses_more_than_1024_buckets(gpu):
    """A gamma range of 5.2 is 1040 buckets: refused, not truncated (1024, above, is accepted)."""
    eng = _empirical_engine(N=2)
    g = np.random.default_rng(92)
    wide = g.uniform(0, 5.2, 5000)
    wide[:2] = 0.0, 5.2
    ok = (g.uniform(0.4, 0.6, 500), g.normal(0, 0.1, 500))
    with pytest.raises(NotImplementedError, match="gamma buckets"):
        eng.empirical_update(_fill_shading(eng, {0: ok, 1: (wide, g.normal(0, 0.1, 5000))}))
    eng.close()


@gpu_test
def test_empirical_update_agents_mask(gpu, oracle):
    """agents= selecting every other edge agent: those equal the oracle, every other agent's
    prev_gamma keeps its bits; a masked-out EmpiricalShadedBidder without a record raises nothing
    (unmasked it is the reference's zero-size error)."""
    eng, cases, per, pg0 = _edge_population(extra=1)
    N = len(pg0)
    mask = np.array([1 if a % 4 == 0 and a < N - 1 else 0 for a in range(N)], np.int32)
    st = _fill_shading(eng, per, seed=6)
    pg = eng.empirical_update(st, agents=mask)
    for j, (name, (gm, ut, _)) in enumerate(cases.items()):
        if mask[2 * j]:
            assert pg[2 * j] == oracle.empirical_update(gm, ut) != pg0[2 * j], name
    off = mask == 0
    assert off[N - 1] and np.array_equal(_bits(pg[off]), _bits(pg0[off]))
    with pytest.raises(ValueError, match="zero-size"):
        eng.empirical_update(st)
    eng.close()


# ---------------------------------------------------------------- 6. the learners' log order is 64 bits
@gpu_test
@pytest.mark.parametrize("base", [(1 << 40) - 300, (1 << 40) - 1024, (1 << 63) - 300],
                         ids=["straddles_2^40", "below_2^40", "straddles_2^63"])
def test_learner_log_order_beyond_40_bits(gpu, oracle, monkeypatch, base):
    """A DoublyRobustBidder and a PolicyLearningBidder on 300 records each whose orders start at
    `base` (the records shuffled in the store): sort_records puts them in log order by all 64 bits
    of `order`, so the trained models equal the oracle on the records in true order, bit for bit.
    Orders that straddle 2^40 (a key of agent << 40 | order's low 40 bits put the later records
    first), orders with bits 10..39 set, and orders that straddle 2^63 (unsigned)."""
    def rebased(eng, recs):
        order = [(np.uint64(base) + np.asarray(o).astype(np.uint64)).view(np.int64) for o in recs["order"]]
        return _learner_store(eng, {**recs, "order": order})
    monkeypatch.setattr(tb, "_learner_store", rebased)
    got = tb._check_run(oracle, monkeypatch, tb.run([tb.learner("dr", 0, 300), tb.learner("ips", 0, 300)], ("train", 0, -1)))
    assert not got["stat"].any() and got["ep"][:, 2].all()
