"""The per-call plugin surface beyond one request of agent 0 (needs an MI355X; `-m gpu`).

ag_estimate_ctr and ag_bid (csrc/ag_plugin.hip: k_estimate_oracle<D>, k_estimate_lrts, k_bid) against
their statement in the oracle's scalars (tests/plugin_reference.py), bit for bit: float64 outputs are
compared as int64 words with NaNs in the same places, and nothing here has a tolerance. The
population, the requests and the conditions they are there for are those of
tests/test_plugin_reference.py, which checks them without a GPU; every case asserts its conditions
on the statement's outputs before it calls the device.

  a. every bidder kind and learner state, every agent of a six-agent population, n in {1, 63, 257,
     4099}: the per-agent offsets of the learner rows, states and shading parameters, the grid's
     stride n, the clip, both softplus branches, propensities of exactly 0;
  b. all 4000 'search' bids of one agent of search_bid_kat.npz in one call, grids sorted and shuffled;
  c. the second pass of the grid-stride loops (4096 workgroups of 256 and a few elements more);
  d. k_estimate_oracle<D> at every D = 2..16, agent 1 of two, the outputs' neighbours untouched;
  e. k_estimate_lrts at model widths 1, 5 and AG_LRTS_MAX_DO with and without Thompson noise;
  f. ag_bid's argument checks and the learner state it reads at call time;
  g. the Python bidders (Bidder.py through plugin_gpu.shading_bid) in their fitted states.
"""
import ctypes
import re

import numpy as np
import pytest

import plugin_reference as R
from test_plugin_reference import (ALLOCATORS, BRANCH_POLICY, CALL_SIZES, E, K, KINDS, MODES, N, OE, P, SEED, STATES,
                                   assert_same_bits, bid_reference, bid_requests, check_bid_case, population,
                                   search_kat)

pytestmark = pytest.mark.gpu

SENTINEL = -1.2345e300  # no CTR, bid, shading factor or density of these inputs
CAP = 4096 * 256        # threads of the largest launch (grid_of)
DRAWS = ("gamma_raw", "eps", "grid")


@pytest.fixture(scope="module")
def pop_engine(gpu, oracle):
    """The six-agent population of tests/test_plugin_reference.py on the device."""
    from auctiongym_amd.engine import AuctionEngine
    pop = population()
    eng = AuctionEngine(N, P, K, E, OE, 1, 1.0)
    eng.set_agent_params(ALLOCATORS, KINDS, pop["prev_gamma"], pop["gamma_sigma"])
    eng.load_catalog(pop["items"], pop["values"])
    eng.load_lrts(pop["ts_m"], pop["ts_q"])
    eng.set_dr_state(pop["dr_state"], STATES)
    eng.set_bidder_modes(MODES)
    yield eng
    eng.close()


def _host(t):
    return t.cpu().numpy()


def _requests(agent, n):
    """The agent's first n requests (copies: the pool is read-only)."""
    return {k: v[:n].copy() for k, v in bid_requests(agent).items()}


def _filled(eng, shape, dtype=None):
    import torch
    return torch.full(shape, SENTINEL, dtype=dtype or torch.float64, device=eng.device)


def _raw_bid(eng, agent, n, value, ctr, gamma_raw, eps, grid, bid, gamma, prop):
    """ag_bid on device tensors (None: NULL); grid already [128][n]. Returns the status."""
    from auctiongym_amd.engine import _ptr, _stream
    return eng.L.ag_bid(eng._h, int(agent), int(n), _ptr(value), _ptr(ctr), _ptr(gamma_raw), _ptr(eps), _ptr(grid),
                        _ptr(bid), _ptr(gamma), _ptr(prop), _stream())


def _raw_estimate(eng, agent, n, x, noise, out_ptr):
    from auctiongym_amd.engine import _ptr, _stream
    return eng.L.ag_estimate_ctr(eng._h, int(agent), int(n), _ptr(x), _ptr(noise), ctypes.c_void_p(out_ptr), _stream())


def _assert_outputs(got, want, n, what):
    for name, g, w in zip(("bid", "gamma", "propensity"), got, want):
        assert_same_bits(_host(g), w[:n], (what, name))


# ---------------------------------------------------------------- a. every state, every agent, n > 1
@pytest.mark.parametrize("n", CALL_SIZES)
@pytest.mark.parametrize("agent", range(N))
def test_bid_every_kind_and_state_at_every_agent(pop_engine, agent, n):
    """eng.bid(agent, ...) for the agent's first n requests, every draw passed whatever its state
    uses: bid, gamma and propensity are the statement's."""
    check_bid_case(agent, n)
    q = _requests(agent, n)
    got = pop_engine.bid(agent, q["value"], q["ctr"], q["gamma_raw"], q["eps"], q["grid"])
    _assert_outputs(got, bid_reference(agent), n, (agent, n))


# ---------------------------------------------------------------- b. the search, pinned to the reference
def test_search_bids_of_the_reference_in_one_call(gpu, oracle):
    """All 4000 bids of agent 3 of search_bid_kat.npz in one ag_bid call (agent 1 of a two-agent
    engine whose agent 0 holds another agent's win-rate model): the reference's gammas and bids. The
    same with every grid row shuffled by its own permutation: the search does not depend on the
    grid's order."""
    from auctiongym_amd.engine import AuctionEngine
    k, other = search_kat(3), search_kat(0)["wr"]
    n = len(k["value"])
    assert n == 4000 and not np.array_equal(other, k["wr"])
    st = np.zeros((2, 16), np.float32)
    st[0, :4], st[1, :4] = other, k["wr"]
    eng = AuctionEngine(2, 1, 1, 1, 1, 1, 1.0)
    eng.set_agent_params([R.ALLOCATOR_ORACLE] * 2, [R.VALUE_LEARNING] * 2, [0.8, 0.7], [0.1, 0.2])
    eng.set_dr_state(st, [R.SEARCH, R.SEARCH])
    eng.set_bidder_modes([0, 0])
    shuffled = np.random.default_rng(SEED).permuted(k["grid"], axis=1)
    assert not np.array_equal(shuffled, k["grid"]) and np.array_equal(np.sort(shuffled, axis=1), k["grid"])
    for what, grid in (("sorted", k["grid"]), ("shuffled", shuffled)):
        b, gamma, prop = eng.bid(1, k["value"], k["ctr"], gamma_grid=grid)
        assert_same_bits(_host(gamma), k["gamma"], (what, "gamma"))
        assert_same_bits(_host(b), k["bid"], (what, "bid"))
        assert (_host(prop) == 1.0).all()
    assert not np.array_equal(_host(eng.bid(0, k["value"], k["ctr"], gamma_grid=k["grid"])[1]), k["gamma"])
    eng.close()


# ---------------------------------------------------------------- c. the second grid-stride pass
def _edge_indices(n):
    """The first 1024 elements, the last 1024 a first pass reaches, and every one beyond."""
    assert n > CAP
    return np.concatenate([np.arange(1024), np.arange(CAP - 1024, CAP), np.arange(CAP, n)])


def test_bid_second_grid_stride_pass(pop_engine):
    """k_bid at n = 4096 * 256 + 257 for the DoublyRobust agent, uninitialised: no output element
    is left unwritten, gamma is the raw draw and bid the IEEE product (value * ctr) * gamma over the
    whole array, the propensity the oracle's on both sides of the launch's last thread."""
    import torch
    eng, pop, agent = pop_engine, population(), BRANCH_POLICY
    assert KINDS[agent] == R.DOUBLY_ROBUST
    n = CAP + 257
    g = np.random.default_rng([SEED, 100])
    ctr = 1.0 / (1.0 + np.exp(-g.normal(-3.0, 1.0, n)))
    value = g.lognormal(0.1, 0.2, n)
    raw = g.normal(pop["prev_gamma"][agent], pop["gamma_sigma"][agent], n)
    dev = [torch.from_numpy(a).to(eng.device) for a in (value, ctr, raw)]
    out = [_filled(eng, (n,)) for _ in range(3)]
    states = list(STATES)
    states[agent] = R.UNINITIALISED
    eng.set_dr_state(pop["dr_state"], states)
    try:
        eng._check(_raw_bid(eng, agent, n, dev[0], dev[1], dev[2], None, None, *out), "ag_bid")
        b, gamma, prop = (_host(t) for t in out)
    finally:
        eng.set_dr_state(pop["dr_state"], STATES)
    for name, a in (("bid", b), ("gamma", gamma), ("propensity", prop)):
        assert not (a == SENTINEL).any(), name
    assert_same_bits(gamma, raw, "gamma")
    assert_same_bits(b, (value * ctr) * raw, "bid")
    idx = _edge_indices(n)
    want = R.bid(KINDS[agent], R.UNINITIALISED, pop["prev_gamma"][agent], pop["gamma_sigma"][agent],
                 pop["dr_state"][agent], value[idx], ctr[idx], raw[idx])
    assert_same_bits(prop[idx], want[2], "propensity")
    assert_same_bits(b[idx], want[0], "bid at the edges")
    assert (prop > 0).all()


@pytest.mark.parametrize("agent", [2, 3])
def test_estimate_ctr_second_grid_stride_pass(pop_engine, agent):
    """ag_estimate_ctr at K = 12, n = 87401 (n * K just over 4096 * 256 threads) for an Oracle agent
    and an LR-TS agent with Thompson noise: nothing left unwritten, and the statement's CTRs in the
    requests at both ends, around the launch's last thread and in every 997th element."""
    import torch
    eng, pop = pop_engine, population()
    n = 87401
    assert K == 12 and CAP < n * K < CAP + 256
    g = np.random.default_rng([SEED, 101, agent])
    lrts = ALLOCATORS[agent] == R.ALLOCATOR_LRTS
    width = OE if lrts else E
    x = np.concatenate([g.normal(0, 1, (n, width)), np.ones((n, 1))], axis=1)
    noise = (g.normal(0, 1, (n, K, OE + 1)) / np.sqrt(pop["ts_q"][agent])).astype(np.float32) if lrts else None
    out = _filled(eng, (n, K))
    eng._check(_raw_estimate(eng, agent, n, torch.from_numpy(x).to(eng.device),
                             torch.from_numpy(noise).to(eng.device) if lrts else None, out.data_ptr()),
               "ag_estimate_ctr")
    got = _host(out)
    assert not (got == SENTINEL).any() and ((got >= 0) & (got <= 1)).all()
    rows = np.unique(np.concatenate([_edge_indices(n * K), np.arange(0, n * K, 997)]) // K)
    assert rows[0] == 0 and rows[-1] == n - 1 and (CAP - 1) // K in rows and CAP // K in rows
    if lrts:
        want = R.lrts_ctr(pop["ts_m"][agent], x[rows], noise[rows])
    else:
        want = R.oracle_ctr(pop["items"][agent], x[rows])
    assert_same_bits(got[rows], want, agent)


# ---------------------------------------------------------------- d. k_estimate_oracle<D> at every D
@pytest.mark.parametrize("E_", range(1, 16))
def test_oracle_estimate_at_every_width(gpu, oracle, E_):
    """OracleAllocator.estimate_CTR for D = E + 1 = 2..16, K in {1, 5, 12}, n = 301, of agent 1 of two
    agents with different catalogues: the statement's CTRs, and the row before and the row after
    the n * K outputs as they were."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    D, n = E_ + 1, 301
    for K_ in (1, 5, 12):
        g = np.random.default_rng([SEED, 200, E_, K_])
        items = np.concatenate([g.normal(0, 0.5, (2, K_, E_)), g.normal(-3, 0.5, (2, K_, 1))], axis=2)
        x = np.concatenate([g.normal(0, 1, (n, E_)), np.ones((n, 1))], axis=1)
        eng = AuctionEngine(2, 1, K_, E_, 1, 1, 1.0)
        eng.load_catalog(items, np.ones((2, K_)))
        buf = _filled(eng, (n + 2, K_))
        eng._check(_raw_estimate(eng, 1, n, torch.from_numpy(x).to(eng.device), None, buf.data_ptr() + 8 * K_),
                   "ag_estimate_ctr")
        got = _host(buf)
        eng.close()
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (D, K_)
        assert_same_bits(got[1:-1], R.oracle_ctr(items[1], x), (D, K_))


# ---------------------------------------------------------------- e. k_estimate_lrts at the widths' ends
@pytest.mark.parametrize("Do", [1, 5, 8])
def test_lrts_estimate_at_the_ends_of_the_width(gpu, oracle, Do):
    """PyTorchLogisticRegressionAllocator.estimate_CTR at model widths 1 (the intercept alone), 5
    (the sgemv order, with and without remainder rows) and AG_LRTS_MAX_DO; K in {1, 3, 4, 7}, n in
    {1, 130}, MAP and Thompson, of agent 1 of two agents with different models."""
    from auctiongym_amd import _lib
    from auctiongym_amd.engine import AuctionEngine
    assert Do in (1, 5, _lib.LRTS_MAX_DO) and _lib.LRTS_MAX_DO == 8
    for K_ in (1, 3, 4, 7):
        g = np.random.default_rng([SEED, 300, Do, K_])
        m = g.normal(0, 1, (2, K_, Do)).astype(np.float32)
        q = g.uniform(1.0, 400.0, (2, K_, Do)).astype(np.float32)
        eng = AuctionEngine(2, 1, K_, max(Do - 1, 1), Do - 1, 1, 1.0)
        eng.set_agent_params([R.ALLOCATOR_LRTS] * 2, [R.TRUTHFUL] * 2)
        eng.load_lrts(m, q)
        for n in (1, 130):
            x = np.concatenate([g.normal(0, 1, (n, Do - 1)), np.ones((n, 1))], axis=1)
            noise = (g.normal(0, 1, (n, K_, Do)) / np.sqrt(q[1])).astype(np.float32)
            for nz in (None, noise):
                got = _host(eng.estimate_ctr(1, x, nz))
                assert_same_bits(got, R.lrts_ctr(m[1], x, nz), (Do, K_, n, nz is not None))
        eng.close()


# ---------------------------------------------------------------- f. the call's contract
def test_bid_optional_outputs_and_empty_call(pop_engine):
    """gamma and propensity may be NULL: the bid is the same (an uninitialised learner, a policy, a
    search). n = 0 is accepted and writes nothing."""
    import torch
    eng, n = pop_engine, 130
    for agent in (2, 3, 5):
        q = _requests(agent, n)
        dev = {k: eng._dev(v, torch.float32 if k == "eps" else torch.float64) for k, v in q.items()}
        grid = dev["grid"].t().contiguous()
        b = _filled(eng, (n,))
        eng._check(_raw_bid(eng, agent, n, dev["value"], dev["ctr"], dev["gamma_raw"], dev["eps"], grid, b, None, None),
                   "ag_bid")
        assert_same_bits(_host(b), bid_reference(agent)[0][:n], agent)
        b0 = _filled(eng, (4,))
        args = (dev["value"], dev["ctr"], dev["gamma_raw"], dev["eps"], grid)
        assert _raw_bid(eng, agent, 0, *args, b0, None, None) == 0
        assert _raw_bid(eng, agent, 0, None, None, None, None, None, None, None, None) == 0
        torch.cuda.synchronize()
        assert (_host(b0) == SENTINEL).all(), agent


def test_bid_refuses_what_it_cannot_answer(pop_engine):
    """An agent out of range, and a state whose draw is missing, with the messages ag_bid states.
    The draws of other states do not stand in for the missing one."""
    eng, n = pop_engine, 63
    q = _requests(0, n)
    v, c, raw, eps, grid = (q[k] for k in ("value", "ctr") + DRAWS)
    for agent in (-1, N):
        with pytest.raises(ValueError, match=re.escape(f"ag_bid: agent {agent} out of range")):
            eng.bid(agent, v, c, raw, eps, grid)
    for agent in range(N):
        if KINDS[agent] >= R.VALUE_LEARNING and STATES[agent] == R.POLICY:
            with pytest.raises(ValueError, match=re.escape(f"ag_bid: agent {agent} bids from its fitted policy: "
                                                           "needs policy_eps")):
                eng.bid(agent, v, c, gamma_raw=raw, gamma_grid=grid)
        elif STATES[agent] == R.SEARCH:
            with pytest.raises(ValueError, match=re.escape(f"ag_bid: agent {agent} bids by search: needs gamma_grid "
                                                           "[128][n]")):
                eng.bid(agent, v, c, gamma_raw=raw, policy_eps=eps)
        elif KINDS[agent] != R.TRUTHFUL:
            with pytest.raises(ValueError, match=re.escape(f"ag_bid: agent {agent} draws a Gaussian shading factor: "
                                                           "needs gamma_raw")):
                eng.bid(agent, v, c, policy_eps=eps, gamma_grid=grid)
        else:
            b, gamma, prop = eng.bid(agent, v, c)  # a truthful bidder draws nothing
            assert_same_bits(_host(b), v * c, agent)
    with pytest.raises(ValueError, match=re.escape("ag_bid: n < 0")):
        eng._check(_raw_bid(eng, 0, -1, None, None, None, None, None, None, None, None), "ag_bid")


def test_bid_reads_the_learner_state_at_call_time(pop_engine):
    """set_dr_state turns agent 2 (uninitialised) to POLICY: its next bid is the policy's, and
    gamma_raw alone no longer serves; turned back, it shades by gamma_raw again."""
    eng, pop, agent, n = pop_engine, population(), 2, 257
    assert STATES[agent] == R.UNINITIALISED
    q = _requests(agent, n)
    states = list(STATES)
    states[agent] = R.POLICY
    want = R.bid(KINDS[agent], R.POLICY, pop["prev_gamma"][agent], pop["gamma_sigma"][agent], pop["dr_state"][agent],
                 q["value"], q["ctr"], eps=q["eps"])
    assert not np.array_equal(want[1], bid_reference(agent)[1][:n])
    eng.set_dr_state(pop["dr_state"], states)
    try:
        _assert_outputs(eng.bid(agent, q["value"], q["ctr"], q["gamma_raw"], q["eps"]), want, n, "policy")
        with pytest.raises(ValueError, match="needs policy_eps"):
            eng.bid(agent, q["value"], q["ctr"], q["gamma_raw"])
    finally:
        eng.set_dr_state(pop["dr_state"], STATES)
    _assert_outputs(eng.bid(agent, q["value"], q["ctr"], q["gamma_raw"]), bid_reference(agent), n, "back")


# ---------------------------------------------------------------- g. the Python classes, fitted
def test_search_bidder_class_reproduces_the_reference(gpu, oracle):
    """ValueLearningBidder(inference='search') with agent 2's win-rate model and generator state of
    search_bid_kat.npz: its first 50 bid() calls return the reference's bids and log its gammas."""
    from auctiongym_amd.Bidder import ValueLearningBidder
    k = search_kat(2)
    rng = np.random.Generator(np.random.PCG64())
    rng.bit_generator.state = k["rng_state"]
    bd = ValueLearningBidder(rng, 0.2, 0.7, inference="search")
    st = np.zeros(16, np.float32)
    st[:4] = k["wr"]
    bd._load_state16(st)
    bd.model_initialised = True
    bids = [bd.bid(k["value"][j], None, k["ctr"][j]) for j in range(50)]
    assert_same_bits(bids, k["bid"][:50], "bid")
    assert_same_bits(bd.gammas, k["gamma"][:50], "gamma")
    assert bd.propensities == [1.0] * 50


@pytest.mark.parametrize("name", ["ValueLearning", "PolicyLearning", "DoublyRobust"])
def test_policy_bidder_classes_bid_from_the_loaded_policy(gpu, oracle, name):
    """A ValueLearningBidder(inference='policy'), a PolicyLearningBidder and a DoublyRobustBidder with
    a loaded N(0, 0.7) state, model_initialised: 50 bid() calls under torch.manual_seed(s) equal the
    statement's policy bids for the same torch.empty(1).normal_() draws, call by call."""
    import torch
    from auctiongym_amd import Bidder as B
    make, kind = {"ValueLearning": (lambda: B.ValueLearningBidder(None, 0.2, 0.7, inference="policy"),
                                    R.VALUE_LEARNING),
                  "PolicyLearning": (lambda: B.PolicyLearningBidder(None, 0.25, "PPO", 0.8), R.POLICY_LEARNING),
                  "DoublyRobust": (lambda: B.DoublyRobustBidder(None, 0.15, 0.9), R.DOUBLY_ROBUST)}[name]
    g = np.random.default_rng([SEED, 400, kind])
    bd = make()
    st = g.normal(0, 0.7, 16).astype(np.float32)
    bd._load_state16(st)
    bd.model_initialised = True
    assert np.array_equal(bd._state16()[4:], st[4:])
    n, seed = 50, 1000 + kind
    ctr = 1.0 / (1.0 + np.exp(-g.normal(-3.0, 1.0, n)))
    value = g.lognormal(0.1, 0.2, n)
    torch.manual_seed(seed)
    eps = np.array([torch.empty(1).normal_().item() for _ in range(n)], np.float32)
    want = R.bid(kind, R.POLICY, bd.prev_gamma, bd.gamma_sigma, st, value, ctr, eps=eps)
    assert len(set(eps.tolist())) == n and ((want[1] > 0) & (want[1] < 1)).any()
    torch.manual_seed(seed)
    for j in range(n):
        b = bd.bid(value[j], None, ctr[j])
        assert_same_bits([b, bd.gammas[-1], bd.propensities[-1]], [w[j] for w in want], (name, j))
    assert len(bd.gammas) == len(bd.propensities) == n
