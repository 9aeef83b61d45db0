"""The host side of the learning bidders' trainers (csrc/ag_dr.hip over csrc/ag_train_host.h): the
plan of ag_bidder_update's launches and the workspaces that grow on demand, against the oracle bit
for bit as tests/test_gpu_trainer_branches.py does, whose tables and helpers these tests use.

Exact-sum learners only (ValueLearning, DoublyRobust): their result does not depend on how the
records are split over workgroups, so one oracle fit stands for every plan. The resident grid is
shared out among more workgroups than fit; the share-out falls back to one workgroup per learner;
the sort buffer and the workgroup tables grow and are reused; ag_bidder_rp_begin .. _end and
ag_lrts_rp_begin .. _end run three times on one context, on more and then fewer workgroups and
barrier lines. tests/host/train_host_check.cpp checks the same planner without a GPU.
"""
import numpy as np
import pytest

import lrts_edge_cases as E
from test_gpu_lrts_edges import _assert_agent, _cus, _samples
from test_gpu_parity import _learner_store
from test_gpu_rp import _rp_run
from test_gpu_shapes import _fill_store, _lrts_engine
from test_gpu_trainer_branches import (_FIELDS, KINDS, SEED, _check_agent, _oracle_fits, _population,
                                       learner)

pytestmark = pytest.mark.gpu

FIXTURE = 1350  # records every agent of the update fixtures has; longer rows lay them end to end again


def _rows(rows, tag):
    """Table rows of this file: `tag` keeps their oracle fits (cached by row) apart from every
    other test's, since here a row's models may come from an earlier update."""
    return [dict(c, tag=tag) for c in rows]


def _pop(rows):
    """test_gpu_trainer_branches._population for rows of any length."""
    bk, modes, state0, init, recs = _population([dict(c, n=min(c["n"], FIXTURE)) for c in rows])
    for a, c in enumerate(rows):
        if c["n"] > FIXTURE:
            for f in _FIELDS:
                recs[f][a] = np.resize(recs[f][a], c["n"])
            recs["order"][a] = len(rows) * np.arange(c["n"]) + a
    return bk, modes, state0, init, recs


def _engine(bk, modes, block):
    from auctiongym_amd.engine import AuctionEngine
    N = len(bk)
    eng = AuctionEngine(N, 2, 12, 5, 4, 0, 1.0)
    eng.set_agent_params(np.zeros(N, np.int32), bk, np.ones(N), np.full(N, 0.02))
    eng.set_bidder_modes(modes)
    eng.set_fit_noise_seed(SEED)
    eng.set_bidder_block_samples(block)
    return eng


def _train(eng, rows, state0, init, recs, mask=None, trace=True):
    """ag_bidder_update of `rows` from (state0, init): what test_gpu_trainer_branches._update returns."""
    N = len(rows)
    eng.set_dr_state(state0, init)
    ep, stat, *tr = eng.bidder_update(_learner_store(eng, recs), None, np.zeros(N, np.int64), 0, trace=trace,
                                      agents=mask)
    state, ini = eng.dr_state()
    return dict(ep=ep, stat=stat, tr=tr[0].cpu().numpy() if trace else None, state=state, ini=ini,
                mask=np.ones(N, np.int32) if mask is None else mask)


def _check(oracle, rows, got, state0, recs, agents=None):
    """The updated agents (or only `agents` of them) against the oracle's fits, bit for bit."""
    sel = got["mask"] if agents is None else got["mask"] & np.isin(np.arange(len(rows)), agents)
    fits = _oracle_fits(oracle, rows, dict(got, mask=sel), state0, recs)
    assert sum(f is not None for f in fits) == sel.sum()
    for a, c in enumerate(rows):
        if fits[a] is not None:
            _check_agent(c, a, got, state0, fits[a])


def _shared_out(sizes, resident, chunk=1):
    """train_plan's workgroups per learner with `chunk` records per workgroup asked for, restated:
    one per chunk; more than the resident grid holds: scaled by resident / wanted, at least one."""
    nblk = [-(-n // chunk) for n in sizes]
    if sum(nblk) > resident:
        nblk = [max(1, int(b * (resident / sum(nblk)))) for b in nblk]
    return nblk


def test_bidder_grid_shared_out(gpu, oracle, monkeypatch):
    """One record per workgroup wanted, for more records than the device holds workgroups (the
    resident grid of either phase is a whole number of workgroups per CU, 8 at the most): both
    launches share their grid out. Two ValueLearning learners ('policy' and 'search') at 45 % each
    of 8 * CUs + 248 records, a DoublyRobust one at 10 % and a ValueLearning one with a single record
    (the oracle's fit of a DoublyRobust learner at 45 % alone takes 7 s).
    The share-out's arithmetic, restated, shows that for every possible resident grid these sizes
    stay in the share-out: they fit, several workgroups to a learner, and never reach the refusal
    (or the fall-back to one workgroup per learner)."""
    cus = _cus(gpu)
    total = 8 * cus + 248
    sizes = (total * 45 // 100, total * 45 // 100, total - 2 * (total * 45 // 100), 1)
    assert max(sizes) <= FIXTURE
    for per_cu in range(1, 9):
        resident = per_cu * cus
        assert sum(sizes) > resident
        nblk = _shared_out(sizes, resident)
        assert sum(nblk) <= resident and max(nblk) > 16 and nblk[3] == 1, (per_cu, nblk)
    monkeypatch.setenv("AG_BIDDER_PIPE", "0")
    rows = _rows([learner("dm", 2, sizes[0]), learner("dm", 0, sizes[1], mode="search"), learner("dr", 1, sizes[2]),
                  learner("dm", 2, sizes[3])], "shared_out")
    bk, modes, state0, init, recs = _pop(rows)
    eng = _engine(bk, modes, 1)
    got = _train(eng, rows, state0, init, recs)
    eng.close()
    _check(oracle, rows, got, state0, recs)


def test_bidder_share_out_falls_back_to_one_workgroup_per_learner(gpu, oracle, monkeypatch):
    """8 * CUs + 1 ValueLearning learners of one record (one workgroup each, which the share-out
    cannot scale down) beside one of 200 records that wants 100 workgroups: the shared-out grid
    would still exceed the resident one, so every learner trains on one workgroup in a plain launch
    instead of the update being refused. Every learner trains (dm_update_kat agent 2 wins its first
    record); the big one and four small ones equal the oracle."""
    from auctiongym_amd import _lib
    N = 8 * _cus(gpu) + 2
    monkeypatch.setenv("AG_BIDDER_PIPE", "0")
    few = _rows([learner("dm", 2, 1), learner("dm", 2, 200)], "fall_back")
    _, _, s2, _, r2 = _pop(few)
    bk = np.full(N, KINDS["dm"], np.int32)
    modes = np.full(N, _lib.VL_POLICY, np.int32)
    state0 = np.repeat(s2[:1], N, axis=0)
    init = np.zeros(N, np.int32)
    recs = {f: [r2[f][0]] * (N - 1) + [r2[f][1]] for f in _FIELDS}
    recs["agent"] = [np.full(len(recs["ctr"][a]), a) for a in range(N)]
    recs["order"] = [N * np.arange(len(recs["ctr"][a])) + a for a in range(N)]
    rows = [few[0]] * (N - 1) + [few[1]]
    eng = _engine(bk, modes, 2)
    got = _train(eng, rows, state0, init, recs, trace=False)  # (the traces of 8 * CUs learners: 1 GB)
    eng.close()
    assert (got["stat"] == 0).all() and (got["ep"][:, 0] > 0).all() and (got["ini"] == _lib.LEARNER_POLICY).all()
    _check(oracle, rows, got, state0, recs, agents=(0, 1, N // 2, N - 2, N - 1))


def test_bidder_workspace_grows_and_is_reused(gpu, oracle, monkeypatch):
    """Three ag_bidder_update calls on one engine at 64 records per workgroup, each from the models
    and flags the previous one left: about 300, then 2400 (the fixtures' 1350 records laid end to
    end again; the sort buffer and the workgroup tables grow), then 150 records per agent (both
    reused, larger than needed). Two DoublyRobust and two ValueLearning learners ('policy' and
    'search'), against the oracle chained the same way. 3 s, most of it the oracle's fits of the
    second update."""
    monkeypatch.setenv("AG_BIDDER_PIPE", "0")
    kinds = (("dr", 0, None), ("dm", 2, "policy"), ("dr", 1, None), ("dm", 0, "search"))
    eng, state0, init = None, None, None
    for round_, base in enumerate((300, 2400, 150)):
        rows = _rows([learner(k, j, base + a, mode=m) for a, (k, j, m) in enumerate(kinds)], f"grows{round_}")
        bk, modes, s0, i0, recs = _pop(rows)
        if eng is None:
            eng, state0, init = _engine(bk, modes, 64), s0, i0
        rows = [dict(c, init=int(init[a])) for a, c in enumerate(rows)]
        got = _train(eng, rows, state0, init, recs)
        _check(oracle, rows, got, state0, recs)
        state0, init = got["state"], got["ini"]
    eng.close()


def test_bidder_rp_begin_twice_on_one_context(gpu, oracle, monkeypatch):
    """ag_bidder_rp_begin .. _end three times on one context, each from what the run before left:
    2 of 72 learners (2 workgroups, 2 barrier lines), then all 72 (past the first run's tables and
    lines, which are allocated with 64 and 16 to spare), then 3. One workgroup per learner (two
    need 2049 records, 6 s of oracle; tests/test_gpu_rp.py has them). Each run equals the persistent trainer (ag_bidder_update on a second engine from the
    same models) in epochs, status, models and flags, and the oracle."""
    monkeypatch.setenv("AG_BIDDER_PIPE", "0")
    N = 72
    kinds = [("dm", a % 3, "search") for a in range(N)]
    kinds[1], kinds[5], kinds[7] = ("dr", 1, None), ("dm", 2, "policy"), ("dr", 0, None)
    rows = _rows([learner(k, j, 30 + a, mode=m) for a, (k, j, m) in enumerate(kinds)],
                 "rp_twice")
    bk, modes, state0, init, recs = _pop(rows)
    eng, twin = _engine(bk, modes, 0), _engine(bk, modes, 0)
    eng.set_dr_state(state0, init)
    st = _learner_store(eng, recs)
    for who in ((1, 4), range(N), (5, 7, 9)):
        mask = np.zeros(N, np.int32)
        mask[list(who)] = 1
        cur = [dict(c, init=int(init[a])) for a, c in enumerate(rows)]
        want = _train(twin, cur, state0, init, recs, mask=mask)
        (ep, stat), = _rp_run([eng], [st], mask)
        state, ini = eng.dr_state()
        got = dict(ep=ep, stat=stat, tr=None, state=state, ini=ini, mask=mask)
        for f in ("ep", "stat", "state", "ini"):
            assert np.array_equal(got[f], want[f]), (list(who), f)
        _check(oracle, cur, got, state0, recs)
        state0, init = state, ini
    eng.close()
    twin.close()


def test_lrts_rp_begin_twice_on_one_context(gpu, oracle):
    """The same for ag_lrts_rp_begin .. _end: 2 of 72 agents, then all 72 with one on two workgroups
    (2148 samples, one workgroup per 2048), then 3; each run from the posterior the one before
    left, equal to the persistent trainer (ag_lrts_update on a second engine holding only the
    masked agents' samples) and to the oracle."""
    import torch
    N, K, Do = 72, 3, 2
    g = np.random.default_rng(54)
    cases = [E.ordinary(g, 2148 if a == 2 else 30 + a, K, Do) for a in range(N)]
    m, q, pm = (np.stack([c[f] for c in cases]) for f in ("m", "q", "pm"))
    eng, twin = _lrts_engine(N, K, Do), _lrts_engine(N, K, Do)
    eng.load_lrts(m, q, pm, thompson_sampling=True)
    st = _fill_store(eng, {a: _samples(c) for a, c in enumerate(cases)})
    for round_, who in enumerate(((1, 4), range(N), (5, 7, 9))):
        mask = np.zeros(N, np.int32)
        mask[list(who)] = 1
        twin.load_lrts(m, q, pm, thompson_sampling=True)
        ep_t = twin.lrts_update(_fill_store(twin, {a: _samples(cases[a]) for a in who}, seed=round_ + 1))
        want = twin.lrts_state()
        eng.lrts_rp_begin(st, agents=mask)
        left, launched = len(list(who)), 0
        while left and launched < E.MAX_EPOCHS + 2:
            eng.lrts_rp_epoch(256)
            launched += 256
            torch.cuda.synchronize()
            left = eng.lrts_rp_poll()
        assert left == 0, (round_, launched)
        got = (eng.lrts_rp_end(), None, eng.lrts_state())
        assert np.array_equal(got[0][mask == 1], ep_t[mask == 1]), round_
        assert all(np.array_equal(x, y) for x, y in zip(got[2], want)), round_
        for a in who:
            _assert_agent(got, a, oracle.lrts_update(*_samples(cases[a]), m[a], pm[a], q[a]), (round_, a))
        m, q, pm = got[2]
    eng.close()
    twin.close()
