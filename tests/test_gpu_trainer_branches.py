"""The learning-bidder trainers' branches the rest of the GPU suite never takes (csrc/ag_dr.hip:
k_bidder_train<0/1>, k_bidder_epoch, k_bidder_pipe), against the oracle bit for bit.

Every other GPU test that trains a learning bidder starts from uninitialised learners, PPO,
ValueLearningBidder 'policy' and the reference's 1350 records per agent. Here: every
PolicyLearningBidder loss on a first and a later update, later DoublyRobustBidder updates (no
imitation fit) in all three kernels, a ValueLearningBidder 'search' update (win-rate fit only, the
policy words untouched, LEARNER_SEARCH afterwards), the NaN exit of the policy fit, and record
counts of 1, 2, 255, 257 and 300, on workgroups with fewer records than threads (even and ragged
slices) and with record caches smaller than the chunk.

Records are prefixes of the committed update fixtures (tests/golden/{ips,dm,dr}_update_kat.npz,
dr_later_kat.npz). The shape is AuctionEngine(N, 2, 12, 5, 4, 0, 1.0); the rsample noise is the
device's synthetic noise (set_fit_noise_seed), the oracle is fed oracle.fit_noise of the same seed
and agent, one epoch more than the device reports (a fit the oracle would run longer ends one
epoch later and fails the epoch comparison). The case tables below are plain data;
test_trainer_table_covers_every_branch (no GPU) checks what they cover.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_00_configs_gpu import _compare
from test_gpu_parity import _kat_learners, _learner_store
from test_gpu_rp import _rp_run
from test_gpu_shapes import _ALL_FIELDS, _catalogue, _rounds, _simulate, _upload
from test_oracle_golden import _dr_later

gpu_test = pytest.mark.gpu  # (per test: the table test below runs without a GPU)

SEED = 5                  # set_fit_noise_seed / oracle.fit_noise
LOSSES = ("REINFORCE", "REINFORCE_offpolicy", "TRPO", "PPO")
KINDS = {"dm": 2, "ips": 3, "dr": 4}  # ValueLearning, PolicyLearning, DoublyRobust (BIDDER_*)
EXACT_SUM_KINDS = ("dm", "dr")        # the learners k_bidder_epoch and k_bidder_pipe train
KAT = {"ips": "ips_update_kat.npz", "dm": "dm_update_kat.npz", "dr": "dr_update_kat.npz"}
LATER = "dr_later_kat.npz"            # iteration-1 records with the reference's own fitted models


def learner(kind, agent, n=300, init=0, mode=None, src=None, nan_at=None, masked=False):
    """One row of a population: `n` first records of `src` agent `agent`. init: the LEARNER_* flag
    loaded before the update (a PolicyLearningBidder with init starts from pol_init_*, a
    dr_later learner from winrate_model0 / bidding_policy0). mode: the PolicyLearningBidder loss or
    the ValueLearningBidder inference ('policy' / 'search'). nan_at: utility[nan_at] = NaN.
    masked: left out of the update by agents=."""
    if mode is None:
        mode = {"ips": "PPO", "dm": "policy", "dr": None}[kind]
    return dict(kind=kind, src=src or KAT[kind], agent=agent, n=n, init=init, mode=mode, nan_at=nan_at,
                masked=masked)


# way: "train" k_bidder_train (ag_bidder_update), "epoch" k_bidder_epoch (one launch per epoch,
# ag_bidder_rp_*: the exact-sum learners of the population, a PolicyLearningBidder's float sums are
# refused there), "pipe" k_bidder_pipe (AG_BIDDER_PIPE=1). variant: (way, block samples, record cache)
def run(learners, *variants):
    return dict(learners=list(learners), variants=list(variants))


# 1. every loss x {first update from pol0_*, later update from pol_init_*}, one launch of 8 agents;
#    the initialised half again on two workgroups of 150 records
PL_LOSS_RUN = run([learner("ips", a % 3, init=a // 4, mode=LOSSES[a % 4]) for a in range(8)], ("train", 0, -1))
PL_SPLIT_RUN = run(PL_LOSS_RUN["learners"][4:], ("train", 200, -1))

# 2. later DoublyRobust updates beside a first one, four ways
DR_LATER_RUN = run([learner("dr", a, init=1, src=LATER) for a in range(3)] + [learner("dr", 0)],
                   ("train", 0, -1), ("train", 200, -1), ("epoch", 0, -1), ("pipe", 0, -1))

# 3. ValueLearningBidder 'search' beside 'policy'
VL_SEARCH_RUN = run([learner("dm", 0, mode="search"), learner("dm", 2)],
                    ("train", 0, -1), ("epoch", 0, -1), ("pipe", 0, -1))


# 4. record-count edges: one PPO, one DR, one 'policy' ValueLearning learner per count
def _trio(n, dm_init=0):
    return [learner("ips", 0, n), learner("dr", 0, n), learner("dm", 0, n, init=dm_init)]


EDGE_RUNS = {
    "n1": run(_trio(1), ("train", 0, -1)),          # (the DR learner's 32768 win-rate epochs: k_bidder_train only)
    "n1_epoch": run([learner("dm", 0, 1), learner("dm", 2, 1)], ("epoch", 0, -1)),
    "n2": run(_trio(2), ("train", 0, -1), ("epoch", 0, -1)),
    "n255": run(_trio(255), ("train", 0, -1), ("epoch", 0, -1)),
    "n257": run(_trio(257), ("train", 0, -1), ("epoch", 0, -1), ("train", 256, -1)),  # 129 + 128 records
    "n300_block256": run(_trio(300), ("train", 256, -1)),   # two workgroups, split evenly: 150 + 150
    "n300_block40": run(_trio(300), ("train", 40, -1)),     # eight workgroups: 7 x 38 records, then 34
    "n300_cache64": run(_trio(300), ("train", 0, 64)),
    "n300_cache0": run(_trio(300, dm_init=1), ("train", 0, 0)),
}
# one learner with records, one masked out (its state and flag stay), one ValueLearningBidder without logs
MASKED_RUN = run([learner("dr", 1), learner("ips", 1, init=1, mode="TRPO", masked=True), learner("dm", 1, 0, init=1)],
                 ("train", 0, -1))

# 5. the NaN exit of the policy fit: an initialised PolicyLearningBidder with one NaN utility, beside a clean one
NAN_RUNS = {loss: run([learner("ips", 0, init=1, mode=loss, nan_at=5), learner("ips", 1, init=1, mode="PPO")],
                      ("train", 0, -1)) for loss in LOSSES}


def slices(n, block):
    """Records per workgroup of k_bidder_train with `block` samples per workgroup (train_plan's
    ceil(n / block) workgroups, wg_slice's even split of ceil(n / workgroups) each)."""
    G = -(-n // block)
    per = -(-n // G)
    return [min(per, n - r * per) for r in range(G)]


ALL_RUNS = [PL_LOSS_RUN, PL_SPLIT_RUN, DR_LATER_RUN, VL_SEARCH_RUN, MASKED_RUN, *EDGE_RUNS.values(), *NAN_RUNS.values()]


def test_trainer_table_covers_every_branch():
    """The tables above (no GPU needed): every (bidder kind, initialised) pair, every
    PolicyLearningBidder loss on a first and on a later update, both ValueLearningBidder modes,
    record counts 1, 2, 255, 257 and 300, all three kernels for each exact-sum learner kind, a
    later DoublyRobust update in every kernel, a 'search' update in every kernel, a second
    workgroup with fewer records than threads, and record caches of 0 and 64."""
    rows = [(c, v) for r in ALL_RUNS for c in r["learners"] for v in r["variants"]]
    assert {(c["kind"], bool(c["init"])) for c, _ in rows} == {(k, i) for k in KINDS for i in (False, True)}
    assert {(c["mode"], c["init"]) for c, _ in rows if c["kind"] == "ips" and c["nan_at"] is None and not c["masked"]} \
        >= {(m, i) for m in LOSSES for i in (0, 1)}
    assert {c["mode"] for c, _ in rows if c["kind"] == "ips" and c["nan_at"] is not None} == set(LOSSES)
    assert {c["mode"] for c, _ in rows if c["kind"] == "dm"} == {"search", "policy"}
    for kind in KINDS:
        assert {c["n"] for c, _ in rows if c["kind"] == kind} >= {1, 2, 255, 257, 300}, kind
    ways = {"train", "epoch", "pipe"}
    for kind in EXACT_SUM_KINDS:
        assert {v[0] for c, v in rows if c["kind"] == kind and c["n"] > 0} == ways, kind
        for n in (2, 255, 257):
            assert {v[0] for c, v in rows if c["kind"] == kind and c["n"] == n} >= {"train", "epoch"}, (kind, n)
    assert {v[0] for c, v in rows if c["kind"] == "dr" and c["init"]} == ways
    assert {v[0] for c, v in rows if c["kind"] == "dr" and not c["init"] and c in DR_LATER_RUN["learners"]} == ways
    assert {v[0] for c, v in rows if c["mode"] == "search"} == ways
    assert {(v[1], v[2]) for c, v in rows if c["n"] == 300} >= {(0, -1), (200, -1), (256, -1), (0, 64), (0, 0)}
    # workgroups with fewer records than their 256 threads, even and ragged slices
    assert slices(300, 256) == [150, 150] and slices(257, 256) == [129, 128] and slices(300, 40) == [38] * 7 + [34]
    assert {(c["n"], v[1]) for c, v in rows} >= {(300, 256), (257, 256), (300, 40)}
    assert any(c["masked"] for c, _ in rows) and any(c["n"] == 0 and c["kind"] == "dm" for c, _ in rows)


# ---------------------------------------------------------------- populations and the oracle
_FIELDS = ("agent", "gamma", "utility", "ctr", "value", "propensity", "won", "order")


def _population(learners):
    """Table rows -> engine inputs: bidder kinds, modes, state0 [N][16], flags [N], records
    {field: [per agent]} cut to each row's prefix."""
    from auctiongym_amd import _lib
    N = len(learners)
    bk = np.array([KINDS[c["kind"]] for c in learners], np.int32)
    modes = np.zeros(N, np.int32)
    state0 = np.zeros((N, 16), np.float32)
    init = np.array([c["init"] for c in learners], np.int32)
    recs = {f: [] for f in _FIELDS}
    for a, c in enumerate(learners):
        n = c["n"]
        if c["src"] == LATER:
            k, (ctr, value, gamma, prop, won, util) = _dr_later(np.load(os.path.join(GOLDEN, LATER)), 1, c["agent"])
            one = dict(ctr=ctr, value=value, gamma=gamma, propensity=prop, won=won, utility=util)
            state0[a, :4], state0[a, 4:] = k("winrate_model0").ravel(), k("bidding_policy0").ravel()
        else:
            _, _, s0, r, (k,) = _kat_learners([(c["kind"], c["src"], c["agent"])])
            one = {f: r[f][0] for f in _FIELDS}
            state0[a] = s0[0]
            if c["kind"] == "ips" and c["init"]:
                state0[a, 4:] = np.concatenate([k(f"pol_init_{i}").ravel() for i in range(6)])
        if c["kind"] == "ips":
            modes[a] = _lib.PL_LOSSES[c["mode"]]
        elif c["kind"] == "dm":
            modes[a] = _lib.VL_POLICY if c["mode"] == "policy" else _lib.VL_SEARCH
            if c["mode"] == "search":  # words the update must leave as they are
                state0[a, 4:] = (0.25 * (np.arange(12) - 5.5)).astype(np.float32)
        assert n <= len(one["ctr"])
        one = {f: np.array(one[f][:n]) for f in one}
        one["agent"], one["order"] = np.full(n, a), N * np.arange(n) + a
        if c["nan_at"] is not None:
            one["utility"] = one["utility"].astype(np.float64)
            one["utility"][c["nan_at"]] = np.nan
        for f in _FIELDS:
            recs[f].append(one[f])
    return bk, modes, state0, init, recs


_ORACLE = {}  # (row, agent index where the noise depends on it, noise epochs, workgroups) -> the oracle's fit


def _oracle_fit(oracle, c, a, state0, recs, ep2, nblk=1):
    """The oracle's update of table row c as agent a (computed once per distinct fit)."""
    pl = c["kind"] == "ips"
    noisy = c["kind"] == "dr" or (c["kind"] == "dm" and c["mode"] == "policy")
    key = (tuple(sorted((k, v) for k, v in c.items() if k != "masked")), a if noisy else -1,
           int(ep2) if noisy else -1, nblk if pl else 1)
    if key not in _ORACLE:
        ctr, value, gamma, prop, won, util = (recs[f][a] for f in ("ctr", "value", "gamma", "propensity", "won", "utility"))
        z = oracle.fit_noise(SEED, a, int(ep2) + 1, c["n"]) if noisy else None
        if pl:
            r = oracle.pl_update(ctr, value, gamma, prop, util, state0[a, 4:], bool(c["init"]), c["mode"], nblk=nblk)
        elif c["kind"] == "dr":
            r = oracle.dr_update(ctr, value, gamma, prop, won, util, state0[a, :4], state0[a, 4:], bool(c["init"]), z)
        else:
            r = oracle.vl_update(ctr, value, gamma, won, state0[a, :4], state0[a, 4:], c["mode"] == "policy", z)
        _ORACLE[key] = r
    return _ORACLE[key]


def _oracle_fits(oracle, learners, got, state0, recs, block=0):
    """The oracle's fits of every updated agent of a launch, side by side on the host's cores (the
    C restatement keeps no state between calls; ctypes drops the GIL): [fit or None per agent]."""
    from concurrent.futures import ThreadPoolExecutor
    todo = [a for a, c in enumerate(learners) if got["mask"][a] and c["n"] > 0]
    nblk = lambda c: (c["n"] + block - 1) // block if block else 1  # noqa: E731
    with ThreadPoolExecutor(max_workers=8) as pool:
        fits = list(pool.map(lambda a: _oracle_fit(oracle, learners[a], a, state0, recs, got["ep"][a, 2],
                                                   nblk(learners[a])), todo))
    return [fits[todo.index(a)] if a in todo else None for a in range(len(learners))]


def _update(monkeypatch, learners, variant):
    """One update of the population `learners` by `variant` = (way, block samples, record cache) ->
    dict(ep, stat, tr (None on the per-epoch path), state, ini) and what went in."""
    from auctiongym_amd.engine import AuctionEngine
    way, block, cache = variant
    bk, modes, state0, init, recs = _population(learners)
    N = len(learners)
    monkeypatch.setenv("AG_BIDDER_PIPE", "1" if way == "pipe" else "0")
    eng = AuctionEngine(N, 2, 12, 5, 4, 0, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), bk, np.ones(N), np.full(N, 0.02))
    eng.set_dr_state(state0, init)
    eng.set_bidder_modes(modes)
    eng.set_fit_noise_seed(SEED)
    eng.set_bidder_block_samples(block)
    eng.set_bidder_record_cache(cache)
    st = _learner_store(eng, recs)
    mask = np.array([0 if c["masked"] else 1 for c in learners], np.int32)
    tr = None
    if way == "epoch":
        mask &= np.isin(bk, [KINDS[k] for k in EXACT_SUM_KINDS]).astype(np.int32)
        (ep, stat), = _rp_run([eng], [st], mask)
    else:
        ep, stat, tr = eng.bidder_update(st, None, np.zeros(N, np.int64), 0, trace=True,
                                         agents=None if mask.all() else mask)
        tr = tr.cpu().numpy()
    state, ini = eng.dr_state()
    return dict(ep=ep, stat=stat, tr=tr, state=state, ini=ini, mask=mask), (eng, state0, init, recs)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _check_agent(c, a, got, state0, r):
    """Agent a's update against the oracle's fit r, bit for bit: the epochs of the three fits,
    every traced epoch loss, the win-rate model, the policy, the status and the learner flag."""
    from auctiongym_amd import _lib
    ep, tr, state = got["ep"][a], got["tr"], got["state"][a]
    what = (c["kind"], c["src"], c["agent"], c["n"], c["init"], c["mode"])
    assert list(ep) == list(r["epochs"]), (what, list(ep), list(r["epochs"]))
    fallback = bool(r.get("fallback"))
    assert not r.get("nan"), what
    assert got["stat"][a] == (1 if fallback else 0), what
    if c["init"] and c["kind"] != "dm":
        assert ep[1] == 0, what  # a later update skips the imitation fit
    if tr is not None:
        last = {"dm": "pol_losses", "dr": "dr_losses", "ips": "pl_losses"}[c["kind"]]
        for slot, key in ((0, "wr_losses"), (1, "init_losses"), (2, last)):
            if key in r:
                assert len(r[key]) == ep[slot], (what, key)
                assert np.array_equal(tr[a, slot, :ep[slot]], r[key].astype(np.float32)), (what, key)
            if ep[slot] == 0:
                assert not tr[a, slot].any(), (what, slot)  # a fit that did not run writes no trace
    if fallback:
        assert list(ep) == [0, 0, 0] and np.array_equal(_bits(state), _bits(state0[a])), what
        assert got["ini"][a] == _lib.LEARNER_UNINITIALISED, what
        return r
    if c["kind"] == "ips":
        assert np.array_equal(_bits(state[:4]), _bits(state0[a, :4])), what
    else:
        assert np.array_equal(state[:4], r["wr"]), what
    assert np.array_equal(state[4:], r["pol"]), what
    if c["kind"] == "dm" and c["mode"] == "search":
        assert list(ep[1:]) == [0, 0] and np.array_equal(_bits(state[4:]), _bits(state0[a, 4:])), what
        assert got["ini"][a] == _lib.LEARNER_SEARCH, what
    else:
        assert got["ini"][a] == _lib.LEARNER_POLICY, what
    return r


def _check_run(oracle, monkeypatch, r, keep_engine=False):
    """Every variant of a table run: the first against the oracle agent by agent, the others equal
    to the first in epochs, status, models and flags (and against the oracle where they differ by
    design: a PolicyLearningBidder's float sums follow the workgroup split)."""
    first, kept = None, None
    for variant in r["variants"]:
        got, (eng, state0, init, recs) = _update(monkeypatch, r["learners"], variant)
        fits = _oracle_fits(oracle, r["learners"], got, state0, recs, variant[1])
        for a, c in enumerate(r["learners"]):
            if fits[a] is not None:
                _check_agent(c, a, got, state0, fits[a])
        if first is None:
            first = got
        sel = got["mask"].astype(bool) & ~np.array([c["kind"] == "ips" for c in r["learners"]])
        for f in ("ep", "stat", "state", "ini"):
            assert np.array_equal(got[f][sel], first[f][sel]), (variant, f)
        if keep_engine and kept is None:
            kept = eng
        else:
            eng.close()
    return (kept, first) if keep_engine else first


# ---------------------------------------------------------------- 1. PolicyLearningBidder losses
@gpu_test
def test_pl_every_loss_first_and_later_update(gpu, oracle, monkeypatch):
    """One ag_bidder_update launch over 8 PolicyLearningBidders, {REINFORCE, REINFORCE_offpolicy,
    TRPO, PPO} x {uninitialised from pol0_*, initialised from pol_init_*}, 300 records of
    ips_update_kat agent a % 3 (fit_pl's four arms, the TRPO KL term and its 5e-2 gradient;
    `if (!initialised[a])` of the PolicyLearning arm). The oracle's policy fits stop after 6158,
    4958, 16384 (the cap) and 872 epochs on a first update and 9708, 16384, 16384 and 1719 on a
    later one, and every epoch's loss is compared, so a loss falling through to another arm cannot
    pass. Initialised agents run 0 imitation epochs and write no imitation trace."""
    got = _check_run(oracle, monkeypatch, PL_LOSS_RUN)
    assert all(got["ep"][a, 1] > 0 for a in range(4)) and all(got["ep"][a, 1] == 0 for a in range(4, 8))
    assert not got["tr"][4:, 1].any()


@gpu_test
def test_pl_later_update_two_workgroups(gpu, oracle, monkeypatch):
    """The initialised half of the loss table with 200 records per workgroup: two workgroups with
    150-record slices. A PolicyLearningBidder's sums are fixed-order floats and follow the split:
    equal to oracle.pl_update(..., nblk=2)."""
    _check_run(oracle, monkeypatch, PL_SPLIT_RUN)


# ---------------------------------------------------------------- 2. later DoublyRobust updates
@gpu_test
def test_dr_later_update_in_all_three_kernels(gpu, oracle, monkeypatch):
    """DoublyRobustBidder updates with initialised = 1 (300 records of dr_later_kat it1_a{0,1,2},
    the reference's fitted winrate_model0 / bidding_policy0; utilities as
    test_oracle_golden._dr_later computes them) beside a first update (dr_update_kat agent 0) in the
    same launch, so both values of the flag sit side by side: the imitation runs 0 epochs and the DR
    fit starts from the loaded policy. The persistent trainer on one workgroup, on two (200 records
    each), the per-epoch launches (fit_after's kFitEu -> kFitPol) and the pipe give the oracle's
    result and each other's. All four agents stay on the per-epoch path: its launches are the
    longest learner's epochs (the first update: 32768 + 12880 + 2071), about a second."""
    _check_run(oracle, monkeypatch, DR_LATER_RUN)


# ---------------------------------------------------------------- 3. ValueLearningBidder 'search'
@gpu_test
def test_vl_search_update_and_bids(gpu, oracle, monkeypatch):
    """A ValueLearningBidder 'search' update (300 records of dm_update_kat agent 0) beside a 'policy'
    one (agent 2): only the win-rate fit runs (epochs [oracle's, 0, 0]), the 12 policy words stay
    bitwise what was loaded, the flag becomes LEARNER_SEARCH (LEARNER_POLICY for the other) -- in
    k_bidder_train, the per-epoch launches (fit_after's kFitWr -> kFitDone) and the pipe. Then 549
    auctions with a host-made gamma grid equal the oracle's on the updated state and flags: the bid
    path takes up what the update left."""
    from auctiongym_amd import _lib
    eng, got = _check_run(oracle, monkeypatch, VL_SEARCH_RUN, keep_engine=True)
    assert list(got["ini"]) == [_lib.LEARNER_SEARCH, _lib.LEARNER_POLICY]
    N, P, K, E, OE, B = 2, 2, 12, 5, 4, 549
    g = np.random.default_rng(4242)
    items, values = _catalogue(g, N, K, E)
    ctx, part, u = _rounds(g, N, P, E, B)
    ak, bk, pg, gs = np.zeros(N, np.int32), np.full(N, 2, np.int32), np.ones(N), np.full(N, 0.02)
    more = dict(gamma_raw=g.normal(pg[part], gs[part]), policy_eps=g.normal(0, 1, (B, P)).astype(np.float32),
                gamma_grid=g.uniform(0.1, 1.0, (B, P, 128)))
    eng.load_catalog(items, values)
    out, cnt = _simulate(eng, _upload(eng, ctx, part, u, **more), B, _ALL_FIELDS)
    orc = oracle.simulate_pop(0, items, values, ctx, part, u, ak, bk, pg, gs, OE=OE, dr_state=got["state"],
                              dr_init=got["ini"], **more)
    _compare(out, cnt, orc, "bids after a 'search' update")
    gam = np.ascontiguousarray(out["gamma"].cpu().numpy().T)
    searched = part == 0
    assert (gam[searched][:, None] == more["gamma_grid"][searched]).any(axis=1).all()  # a point of its grid
    eng.close()


# ---------------------------------------------------------------- 4. record-count edges
@gpu_test
@pytest.mark.parametrize("name", list(EDGE_RUNS))
def test_record_count_edges(gpu, oracle, monkeypatch, name):
    """One PPO, one DoublyRobust and one 'policy' ValueLearning learner on 1, 2, 255 and 257 records
    (fewer records than the 256 threads of a workgroup, one more) in k_bidder_train and the
    per-epoch launches, on several workgroups with fewer records than threads (the trainer splits an
    agent's records evenly: 256 samples per workgroup give 150 + 150 of 300 and 129 + 128 of 257;
    40 give seven slices of 38 and a ragged one of 34), and with record caches of 64 and 0 records
    under a 300-record chunk. dm_update_kat agent 0 wins neither of its first two records: status 1, epochs
    [0, 0, 0], state unchanged, LEARNER_UNINITIALISED (n1_epoch: beside agent 2, which wins both)."""
    got = _check_run(oracle, monkeypatch, EDGE_RUNS[name])
    if name in ("n1", "n2"):
        assert list(got["stat"]) == [0, 0, 1]
    elif name == "n1_epoch":
        assert list(got["stat"]) == [1, 0]
    else:
        assert not got["stat"].any()


@gpu_test
def test_masked_and_logless_learners(gpu, oracle, monkeypatch):
    """A DoublyRobust learner with records, an initialised PolicyLearningBidder masked out by
    agents= (its state and flag stay bit for bit, nothing is reported for it) and an initialised
    ValueLearningBidder without a record (src/Bidder.py:213-216: falls back, status 1, bids Gaussian
    again)."""
    from auctiongym_amd import _lib
    got, (eng, state0, init, recs) = _update(monkeypatch, MASKED_RUN["learners"], MASKED_RUN["variants"][0])
    eng.close()
    fits = _oracle_fits(oracle, MASKED_RUN["learners"], got, state0, recs)
    assert [f is not None for f in fits] == [True, False, False]
    _check_agent(MASKED_RUN["learners"][0], 0, got, state0, fits[0])
    assert np.array_equal(_bits(got["state"][1]), _bits(state0[1])) and got["ini"][1] == init[1] == 1
    assert list(got["ep"][1]) == [0, 0, 0] and got["stat"][1] == 0 and not got["tr"][1].any()
    assert got["stat"][2] == 1 and list(got["ep"][2]) == [0, 0, 0]
    assert np.array_equal(_bits(got["state"][2]), _bits(state0[2])) and got["ini"][2] == _lib.LEARNER_UNINITIALISED


# ---------------------------------------------------------------- 5. the NaN exit
@gpu_test
@pytest.mark.parametrize("loss", LOSSES)
def test_pl_nan_loss_is_an_error(gpu, oracle, monkeypatch, loss):
    """An initialised PolicyLearningBidder whose utility[5] is NaN: the first epoch's loss is NaN,
    the reference exits (src/Bidder.py:409-417), the oracle returns nan with epochs [0, 0, 1], and
    ag_bidder_update returns an error naming it. What the library leaves behind: k_bidder_train has
    written every trained agent's model before the host reads the status, and the error returns
    before any learner flag is updated -- so the clean agent of the same launch holds the oracle's
    policy and every flag is as loaded."""
    learners = NAN_RUNS[loss]["learners"]
    bk, modes, state0, init, recs = _population(learners)
    r = _oracle_fit(oracle, learners[0], 0, state0, recs, 0)
    assert r["nan"] and list(r["epochs"]) == [0, 0, 1]
    clean = _oracle_fit(oracle, learners[1], 1, state0, recs, 0)
    assert not clean["nan"] and clean["epochs"][2] > 1
    from auctiongym_amd.engine import AuctionEngine
    monkeypatch.setenv("AG_BIDDER_PIPE", "0")
    eng = AuctionEngine(2, 2, 12, 5, 4, 0, 1.0)
    eng.set_agent_params(np.zeros(2, np.int32), bk, np.ones(2), np.full(2, 0.02))
    eng.set_dr_state(state0, init)
    eng.set_bidder_modes(modes)
    st = _learner_store(eng, recs)
    with pytest.raises(ValueError, match="agent 0: PolicyLearningBidder: NAN DETECTED"):
        eng.bidder_update(st, None, np.zeros(2, np.int64), 0)
    state, ini = eng.dr_state()
    assert np.array_equal(state[1, 4:], clean["pol"]) and np.array_equal(_bits(state[1, :4]), _bits(state0[1, :4]))
    assert np.array_equal(ini, init)
    eng.close()
