"""The statement of the per-call plugin surface (tests/plugin_reference.py) pinned to what is
already pinned to the reference, and the population and requests tests/test_gpu_plugin_calls.py
runs on the device, with the conditions they are there for checked here on the CPU.

The population (N = 6, K = 12, E = 5, OE = 4) holds every bidder kind and learner state once, with
allocators alternating Oracle and LR-TS, and nothing shared between agents -- prev_gamma,
gamma_sigma, learner rows (N(0, 0.7)), catalogues and LR-TS models all differ -- so that reading
another agent's row changes the answer:

    agent  bidder            state           allocator
    0      truthful          -               Oracle
    1      EmpiricalShaded   -               LR-TS
    2      ValueLearning     uninitialised   Oracle
    3      PolicyLearning    POLICY          LR-TS
    4      DoublyRobust      POLICY          Oracle    shared-layer biases 25 and -30 (softplus u > 20)
    5      ValueLearning     SEARCH          LR-TS

Each agent has one pool of 4099 requests (bid_requests); a call of n requests takes the first n.
The first rows carry the edges: value 0 and a negative value (rows 0, 1); gamma_raw below 0, above
1, exactly 0 and exactly 1 (rows 2-5); eps +-50, +-40, 0, +-1e-3 and 8 (rows 2-9); every fifth grid
row holds each of 64 points twice. Grids are unsorted.
"""
import functools
import json
import os

import numpy as np
import pytest

import plugin_reference as R
from conftest import GOLDEN

N, P, K, E, OE = 6, 2, 12, 5, 4
KINDS = (R.TRUTHFUL, R.EMPIRICAL_SHADED, R.VALUE_LEARNING, R.POLICY_LEARNING, R.DOUBLY_ROBUST, R.VALUE_LEARNING)
STATES = (R.UNINITIALISED, R.UNINITIALISED, R.UNINITIALISED, R.POLICY, R.POLICY, R.SEARCH)
ALLOCATORS = (R.ALLOCATOR_ORACLE, R.ALLOCATOR_LRTS) * 3
MODES = (0, 0, 1, 3, 0, 0)  # ValueLearning: 1 policy, 0 search; PolicyLearning: 3 PPO
PLAIN_POLICY, BRANCH_POLICY, SEARCH_AGENT, EMPIRICAL_AGENT = 3, 4, 5, 1
# The smallest seed from 5 on at which every call meets check_bid_case (at 5 the plain policy clips 3 %
# of its first 63 requests to 0). The conditions are asserted on every run, here and before each
# device call, so a seed that stopped meeting them would fail, not pass quietly.
SEED = 6
CALL_SIZES = (1, 63, 257, 4099)
POOL = max(CALL_SIZES)
EPS_EDGES = (50.0, -50.0, 40.0, -40.0, 0.0, 1e-3, -1e-3, 8.0)
RAW_EDGES = (-0.25, 1.5, 0.0, 1.0)


def assert_same_bits(got, want, what=""):
    """Equal bit for bit as float64, NaNs in the same places."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN positions")
    g, w = np.ascontiguousarray(got[~nan]), np.ascontiguousarray(want[~nan])
    bad = np.flatnonzero(g.view(np.int64) != w.view(np.int64))
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


@functools.lru_cache(maxsize=None)
def population():
    """The shared population (read-only arrays)."""
    g = np.random.default_rng(SEED)
    pop = dict(
        items=np.concatenate([g.normal(0, 0.5, (N, K, E)), g.normal(-3, 0.5, (N, K, 1))], axis=2),
        values=g.lognormal(0.1, 0.2, (N, K)),
        ts_m=g.normal(0, 1, (N, K, OE + 1)).astype(np.float32),
        ts_q=g.uniform(1.0, 400.0, (N, K, OE + 1)).astype(np.float32),
        prev_gamma=np.array([1.0, 0.9, 0.75, 0.85, 0.65, 0.8]),
        gamma_sigma=np.array([1.0, 0.3, 0.2, 0.25, 0.15, 0.1]),
        dr_state=g.normal(0, 0.7, (N, 16)).astype(np.float32))
    pop["dr_state"][BRANCH_POLICY, 4 + 4] = 25.0   # p[4], p[5]: the shared layer's biases
    pop["dr_state"][BRANCH_POLICY, 4 + 5] = -30.0
    # a win-rate model as steep in gamma as a fitted one (N(0, 0.7) weights always pick the
    # smallest grid point: the utility's factor 1 - gamma decides alone)
    pop["dr_state"][SEARCH_AGENT, 2:4] = 6.0, -4.0
    for a in pop.values():
        a.setflags(write=False)
    return pop


@functools.lru_cache(maxsize=None)
def bid_requests(agent):
    """The agent's pool of POOL requests: value, ctr, gamma_raw [POOL], eps [POOL] float32, grid
    [POOL][128] (read-only)."""
    pop = population()
    g = np.random.default_rng([SEED, agent])
    req = dict(ctr=1.0 / (1.0 + np.exp(-g.normal(-3.0, 1.0, POOL))), value=g.lognormal(0.1, 0.2, POOL),
               gamma_raw=g.normal(pop["prev_gamma"][agent], pop["gamma_sigma"][agent], POOL),
               eps=g.normal(0, 1, POOL).astype(np.float32), grid=g.uniform(0.1, 1.0, (POOL, R.GRID_POINTS)))
    req["value"][0], req["value"][1] = 0.0, -0.75
    req["gamma_raw"][2:2 + len(RAW_EDGES)] = RAW_EDGES
    req["eps"][2:2 + len(EPS_EDGES)] = EPS_EDGES
    for r in range(3, POOL, 5):  # 64 points, each twice, in another order
        req["grid"][r, 64:] = req["grid"][r, :64][g.permutation(64)]
    for a in req.values():
        a.setflags(write=False)
    return req


@functools.lru_cache(maxsize=None)
def bid_reference(agent):
    """(bid, gamma, propensity) [POOL] of the agent's pool by the statement; requests are
    independent, so a call of n requests must give the first n (read-only)."""
    pop, q = population(), bid_requests(agent)
    out = R.bid(KINDS[agent], STATES[agent], pop["prev_gamma"][agent], pop["gamma_sigma"][agent],
                pop["dr_state"][agent], q["value"], q["ctr"], q["gamma_raw"], q["eps"], q["grid"])
    for a in out:
        a.setflags(write=False)
    return out


def shared_layer_inputs(agent, n):
    """u [n][2] of the policy's two softplus units, as policy_bid forms them (float32 ctr and
    value, double arithmetic): the branch softplus(u) = u is taken where u > 20."""
    p = population()["dr_state"][agent, 4:].astype(np.float64)
    q = bid_requests(agent)
    c, v = (q[k][:n].astype(np.float32).astype(np.float64) for k in ("ctr", "value"))
    return np.stack([c * p[0] + v * p[1] + p[4], c * p[2] + v * p[3] + p[5]], axis=1)


def check_bid_case(agent, n):
    """What the agent's first n requests are there for, asserted on the statement's outputs. A
    call of one request holds none of the edges but the value-0 row."""
    q, (_, gamma, prop) = bid_requests(agent), bid_reference(agent)
    gamma, prop = gamma[:n], prop[:n]
    kind, state = KINDS[agent], STATES[agent]
    if kind == R.TRUTHFUL:
        assert np.isnan(gamma).all() and np.isnan(prop).all()
    elif state == R.POLICY:
        u = shared_layer_inputs(agent, n)
        assert np.isfinite(gamma).all() and np.isfinite(prop).all()
        if agent == BRANCH_POLICY:
            assert (u[:, 0] > 20.0).all() and (u[:, 1] < -20.0).all()
        else:
            assert (u <= 20.0).all()
            if n >= 63:
                share = [np.mean(gamma == 0.0), np.mean(gamma == 1.0), np.mean((gamma > 0.0) & (gamma < 1.0))]
                assert min(share) >= 0.05, share
                assert (prop == 0.0).sum() >= 1 and (prop > 0.0).sum() >= n // 2
    elif state == R.SEARCH:
        assert (prop == 1.0).all()
        assert q["value"][0] == 0.0 and gamma[0] == q["grid"][0].min()
        if n >= 2:
            assert q["value"][1] < 0.0 and gamma[1] == q["grid"][1].max()
        if n >= 63:  # not always an end of the grid, and grids with doubled points among them
            rows = np.arange(n)
            inner = (gamma != q["grid"][:n].min(axis=1)) & (gamma != q["grid"][:n].max(axis=1))
            assert inner.mean() >= 0.05 and inner[rows % 5 == 3].any()
    elif kind == R.EMPIRICAL_SHADED:
        assert np.isnan(prop).all()
        if n >= 63:
            raw = q["gamma_raw"][:n]
            assert (raw < 0.0).any() and (raw > 1.0).any() and (raw == 0.0).any() and (raw == 1.0).any()
            assert (gamma[raw < 0.0] == 0.0).all() and (gamma[raw > 1.0] == 1.0).all()
            assert ((gamma > 0.0) & (gamma < 1.0)).any() and gamma.min() == 0.0 and gamma.max() == 1.0
    else:  # an uninitialised learner: the raw draw kept, its Gaussian density logged
        assert np.array_equal(gamma, q["gamma_raw"][:n]) and (prop > 0.0).all()
        if n >= 63:
            assert (gamma < 0.0).any() and (gamma > 1.0).any()


# ---------------------------------------------------------------- the GPU file's cases, on the CPU
def test_population_holds_every_kind_and_state_once_with_nothing_shared():
    pop = population()
    assert sorted(zip(KINDS, STATES)) == sorted([(0, 0), (1, 0), (2, 0), (2, 2), (3, 1), (4, 1)])
    for key in ("items", "values", "ts_m", "ts_q", "dr_state"):
        rows = pop[key].reshape(N, -1)
        assert all(not np.any(rows[a] == rows[b]) for a in range(N) for b in range(a)), key
    shading = [a for a in range(N) if KINDS[a] != R.TRUTHFUL]
    assert len({pop["prev_gamma"][a] for a in shading}) == len({pop["gamma_sigma"][a] for a in shading}) == 5


@pytest.mark.parametrize("n", CALL_SIZES)
@pytest.mark.parametrize("agent", range(N))
def test_bid_cases_meet_their_conditions(oracle, agent, n):
    """Every (agent, n) the GPU file calls takes the branches it is there for."""
    check_bid_case(agent, n)
    b, gamma, _ = bid_reference(agent)
    q = bid_requests(agent)
    if KINDS[agent] != R.TRUTHFUL:
        assert_same_bits(b[:n], (q["value"][:n] * q["ctr"][:n]) * gamma[:n])


# ---------------------------------------------------------------- against the reference's capture
def search_kat(agent):
    """value, ctr, the reference's gamma and bid [4000], its win-rate model [4] and the sorted grids
    [4000][128] it drew (regenerated from the stored generator state) of one agent of
    tests/golden/search_bid_kat.npz."""
    k = np.load(os.path.join(GOLDEN, "search_bid_kat.npz"))
    v, c, gamma, bids, wr = (k[f"a{agent}_{s}"] for s in ("value", "ctr", "gamma", "bid", "wr"))
    rng = np.random.Generator(np.random.PCG64())
    state = json.loads(str(k[f"a{agent}_rng_state"]))
    rng.bit_generator.state = state
    grids = np.stack([np.sort(rng.uniform(0.1, 1.0, size=R.GRID_POINTS)) for _ in range(len(v))])
    return dict(value=v, ctr=c, gamma=gamma, bid=bids, wr=wr.astype(np.float32), grid=grids, rng_state=state)


@pytest.mark.parametrize("agent", range(6))
def test_search_bid_reproduces_the_reference(oracle, agent):
    """The first 500 'search' bids of each agent of search_bid_kat.npz: the reference's gamma and
    bid, with propensity 1."""
    k = search_kat(agent)
    st = np.zeros(16, np.float32)
    st[:4] = k["wr"]
    st[4:] = 9.0  # the policy rows are not the search's business
    b, gamma, prop = R.bid(R.VALUE_LEARNING, R.SEARCH, 0.7, 0.2, st, k["value"][:500], k["ctr"][:500],
                           grid=k["grid"][:500])
    assert_same_bits(gamma, k["gamma"][:500], "gamma")
    assert_same_bits(b, k["bid"][:500], "bid")
    assert (prop == 1.0).all()


# ---------------------------------------------------------------- against the oracle's batched replay
def test_statement_equals_oracle_replay_of_the_population(oracle):
    """oracle.simulate_pop at P = 1 on the population (dense gamma_raw, policy_eps, gamma_grid): the
    statement, given the item the replay chose, gives its est_ctr, bid, gamma and propensity in
    every round."""
    pop = population()
    g = np.random.default_rng(SEED + 1)
    B = 150 * N
    ctx = g.normal(0, 1, (B, E))
    part = g.permutation(np.arange(B) % N).astype(np.int32).reshape(B, 1)
    raw = g.normal(0.8, 0.3, (B, 1))
    eps = g.normal(0, 1, (B, 1)).astype(np.float32)
    grid = g.uniform(0.1, 1.0, (B, 1, R.GRID_POINTS))
    o = oracle.simulate_pop(1, pop["items"], pop["values"], ctx, part, g.random(B), ALLOCATORS, KINDS,
                            pop["prev_gamma"], pop["gamma_sigma"], OE=OE, ts_m=pop["ts_m"], gamma_raw=raw,
                            ts_sample=False, dr_state=pop["dr_state"], dr_init=np.array(STATES, np.int32),
                            policy_eps=eps, gamma_grid=grid)
    x = np.concatenate([ctx, np.ones((B, 1))], axis=1)
    xo = np.concatenate([ctx[:, :OE], np.ones((B, 1))], axis=1)
    for a in range(N):
        rows = np.flatnonzero(part[:, 0] == a)
        item = o["item"][rows, 0]
        if ALLOCATORS[a] == R.ALLOCATOR_ORACLE:
            ctr = R.oracle_ctr(pop["items"][a], x[rows])
        else:
            ctr = R.lrts_ctr(pop["ts_m"][a], xo[rows])
        est = ctr[np.arange(len(rows)), item]
        assert_same_bits(est, o["est_ctr"][rows, 0], (a, "est_ctr"))
        b, gamma, prop = R.bid(KINDS[a], STATES[a], pop["prev_gamma"][a], pop["gamma_sigma"][a], pop["dr_state"][a],
                               pop["values"][a][item], est, raw[rows, 0], eps[rows, 0], grid[rows, 0])
        assert_same_bits(b, o["bid"][rows, 0], (a, "bid"))
        assert_same_bits(gamma, o["gamma"][rows, 0], (a, "gamma"))
        assert_same_bits(prop, o["propensity"][rows, 0], (a, "propensity"))
        assert len(set(item.tolist())) > 1, a  # more than one row of the catalogue / model in play


def test_lrts_statement_adds_the_noise_in_float32(oracle):
    """lrts_ctr(m, x, noise) is the MAP forward of the float32 sum m + noise, request by request."""
    g = np.random.default_rng(SEED + 2)
    m = g.normal(0, 1, (7, 5)).astype(np.float32)
    x = np.concatenate([g.normal(0, 1, (9, 4)), np.ones((9, 1))], axis=1)
    noise = g.normal(0, 0.3, (9, 7, 5)).astype(np.float32)
    got = R.lrts_ctr(m, x, noise)
    assert np.array_equal(got, got.astype(np.float32))  # float32 values, widened
    for i in range(9):
        assert_same_bits(got[i], R.lrts_ctr(m + noise[i], x[i:i + 1])[0], i)
    assert not np.array_equal(got, R.lrts_ctr(m, x))


# ---------------------------------------------------------------- against plain numpy
@pytest.mark.parametrize("D", range(2, 17))
def test_oracle_ctr_within_rounding_of_longdouble(oracle, D):
    """oracle_ctr against the longdouble statement at every catalogue width, unit and large
    coefficients: |difference| <= (D + 1) 2^-53 S / 4 + 4 2^-53 (oracle_ctr_bound)."""
    g = np.random.default_rng(100 + D)
    for scale in (1.0, 6.0):
        items = g.normal(0, scale, (7, D))
        x = np.concatenate([g.normal(0, 1, (200, D - 1)), np.ones((200, 1))], axis=1)
        got = R.oracle_ctr(items, x)
        want = R.oracle_ctr_longdouble(items, x)
        err = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        bound = R.oracle_ctr_bound(items, x)
        assert (err <= bound).all(), (D, scale, float((err / bound).max()))
        assert ((got > 0) & (got <= 1)).all() and got.std() > 0.1
