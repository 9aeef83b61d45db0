"""The LR-TS trainers (csrc/ag_lrts.hip: k_lrts_train, and k_lrts_epoch behind ag_lrts_rp_*) at the
branches the rest of the GPU suite never reaches, against oracle.lrts_update bit for bit: epochs, m, q,
prev_m and, where a trace is taken, every epoch's float32 loss. Nothing is compared with the other
device form, and there is no tolerance anywhere.

The inputs are tests/lrts_edge_cases.py; tests/test_lrts_edge_inputs.py shows on the oracle alone that
each reaches its branch (the epoch cap, a saturated sigmoid, the -100 clamp, ...). Here they meet
the splits: samples streamed past the register cache, a two-level combining tree, a grid shared out
among more workgroups than fit (with empty chunks), the share-out's fall-back to one workgroup per
agent, workspace growth and reuse, and several workgroups per agent in the per-epoch form.
"""
import numpy as np
import pytest

import lrts_edge_cases as E
from test_gpu_shapes import _fill_store, _lrts_engine

pytestmark = pytest.mark.gpu


def _engine(cases, K, Do):
    """An engine of len(cases) LR-TS agents loaded with the cases' priors, and the posteriors (a
    single case gets a second agent without samples: an auction has two participants)."""
    cases = list(cases) * (2 if len(cases) == 1 else 1)
    eng = _lrts_engine(len(cases), K, Do)
    post = [np.stack([c[f] for c in cases]) for f in ("m", "q", "pm")]
    eng.load_lrts(*post, thompson_sampling=True)
    return eng, post


def _samples(c):
    return c["X"], c["A"], c["y"]


def _assert_agent(got, a, want, tag):
    """got: (epochs, trace or None, (m, q, pm)) of the device; want: the oracle's result."""
    ep, tr, (m, q, pm) = got
    om, opm, oq, oep, oL = want
    assert oep > 0 and ep[a] == oep, (tag, a, ep[a], oep)
    if tr is not None:
        assert np.array_equal(tr[a, :oep], np.asarray(oL, np.float32)), (tag, a)
    assert np.array_equal(m[a], om), (tag, a)
    assert np.array_equal(q[a], oq), (tag, a)
    assert np.array_equal(pm[a], opm), (tag, a)


def _update(eng, st, trace=True):
    if not trace:
        return eng.lrts_update(st), None, eng.lrts_state()
    ep, tr = eng.lrts_update(st, trace=True)
    return ep, tr.cpu().numpy(), eng.lrts_state()


# ------------------------------------------------------------------ B. k_lrts_train
@pytest.mark.parametrize("shape", sorted(E.GROUPS), ids=lambda s: f"K{s[0]}xDo{s[1]}")
def test_edge_inputs_persistent_trainer(gpu, oracle, shape):
    """Every edge input of one model shape in one launch (the cases mix in the grid), on one
    workgroup per agent and split over 64-sample workgroups. The cap inputs report 16384 epochs and
    a trace equal in all 16384 columns."""
    names = E.GROUPS[shape]
    cases = [E.case(n) for n in names]
    eng, post = _engine(cases, *shape)
    st = _fill_store(eng, {a: _samples(c) for a, c in enumerate(cases)})
    for chunk in (0, 64):
        eng.set_lrts_block_samples(chunk)
        eng.load_lrts(*post, thompson_sampling=True)
        got = _update(eng, st)
        for a, n in enumerate(names):
            _assert_agent(got, a, E.oracle_result(n), (n, chunk))
            if n in E.CAP:
                assert got[0][a] == E.MAX_EPOCHS and len(E.oracle_result(n)[4]) == E.MAX_EPOCHS
    eng.close()


@pytest.mark.parametrize("name", ["big_k12", "big_k2"])
def test_big_inputs_persistent_trainer(gpu, oracle, name):
    """The two large inputs at the default split and on 64-sample workgroups, with the trace.
    4396 samples at K * (OE + 1) = 60: two workgroups, then 69 (a two-level tree). 34 900 samples:
    nine workgroups, then 546 wanted by ONE agent -- on a device holding fewer, a share-out of
    real data in which every workgroup keeps samples."""
    c = E.case(name)
    eng, post = _engine([c], *c["m"].shape)
    st = _fill_store(eng, {0: _samples(c)})
    for chunk in (0, 64):
        eng.set_lrts_block_samples(chunk)
        eng.load_lrts(*post, thompson_sampling=True)
        got = _update(eng, st)
        _assert_agent(got, 0, E.oracle_result(name), (name, chunk))
        assert got[0][1] == 0 and all(np.array_equal(x[1], p[1]) for x, p in zip(got[2], post))  # no samples
    eng.close()


def test_streamed_samples(gpu, oracle):
    """4396 samples in ONE workgroup (8192 per workgroup allowed): 4096 in registers and 300
    streamed from memory every epoch and in the Laplace pass; then the same store on two
    workgroups of 2198, nothing streamed."""
    c = E.case("big_k12")
    eng, post = _engine([c], 12, 5)
    st = _fill_store(eng, {0: _samples(c)})
    for chunk in (8192, 2200):
        eng.set_lrts_block_samples(chunk)
        eng.load_lrts(*post, thompson_sampling=True)
        _assert_agent(_update(eng, st), 0, E.oracle_result("big_k12"), chunk)
    eng.close()


def test_two_level_tree_beside_smaller_agents(gpu, oracle):
    """16 samples per workgroup: a 100-sample agent on 7 workgroups (the last one short), a
    400-sample agent on 25 (two levels of the combining tree) and a 3-sample agent on one, so
    every agent has its own barrier lines and accumulator rows."""
    names = ("tree_100", "tree_400", "n3")
    cases = [E.case(n) for n in names]
    eng, _ = _engine(cases, 6, 2)
    eng.set_lrts_block_samples(16)
    got = _update(eng, _fill_store(eng, {a: _samples(c) for a, c in enumerate(cases)}))
    for a, n in enumerate(names):
        _assert_agent(got, a, E.oracle_result(n), n)
    eng.close()


def _cus(gpu):
    import torch
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def test_grid_shared_out(gpu, oracle):
    """One sample per workgroup wanted, for more samples than the device holds workgroups (the
    resident grid is some whole number of 256-thread workgroups per CU, 8 at the most; 2 on an
    MI355X at this model size): the grid is shared out, and most workgroups get a few samples or
    none. Three agents at 45 % / 45 % / 10 % of the samples and a fourth with two. The share-out's
    own arithmetic, restated, shows that for every possible resident grid these sizes stay in the
    share-out (they never fall back to one workgroup per agent) and, for nearly all, leave empty chunks."""
    cus = _cus(gpu)
    total = 8 * cus + 248
    g = np.random.default_rng(51)
    sizes = (total * 45 // 100, total * 45 // 100, total - 2 * (total * 45 // 100), 2)
    empty = {}
    for per_cu in range(1, 9):
        resident = per_cu * cus
        assert sum(sizes) > resident
        nblk = [max(1, int(n * (resident / sum(sizes)))) for n in sizes]  # chunk 1: n workgroups wanted
        assert sum(nblk) <= resident and max(nblk) > 16, (per_cu, nblk)   # shared out, never the fall-back
        empty[per_cu] = sum(b - -(-n // -(-n // b)) for n, b in zip(sizes, nblk))
    # workgroups past the end of their agent's samples: under 2 per CU (what an MI355X holds of this
    # kernel) and under all but at most one of the other grids
    assert empty[2] >= 8 and sum(e >= 8 for e in empty.values()) >= 7, empty
    cases = [E.ordinary(g, n, 2, 2) for n in sizes]
    cases[3]["A"][:] = 1
    cases[3]["y"] = np.array([False, True])
    eng, _ = _engine(cases, 2, 2)
    eng.set_lrts_block_samples(1)
    got = _update(eng, _fill_store(eng, {a: _samples(c) for a, c in enumerate(cases)}))
    for a, c in enumerate(cases):
        _assert_agent(got, a, oracle.lrts_update(*_samples(c), c["m"], c["pm"], c["q"]), (a, sizes))
    eng.close()


def test_share_out_falls_back_to_one_workgroup_per_agent(gpu, oracle):
    """8 * CUs + 1 agents of two samples (one workgroup each, which the share-out cannot scale
    down) beside one of 200 samples that wants 100 workgroups: the shared-out grid would still
    exceed the resident one, so every agent trains on one workgroup instead of the update being
    refused. Every agent trains; the big one and four small ones equal the oracle."""
    N = 8 * _cus(gpu) + 2
    g = np.random.default_rng(52)
    m = g.normal(0, 1, (N, 3, 2)).astype(np.float32)
    q = (1 + g.random((N, 3, 2))).astype(np.float32)
    pm = (m + 0.5).astype(np.float32)
    per = {}
    for a in range(N - 1):
        per[a] = (E.features(g, 2, 2), np.full(2, a % 3), np.array([False, True]))
    per[N - 1] = (E.features(g, 200, 2), g.integers(0, 3, 200), g.random(200) < 0.35)
    eng = _lrts_engine(N, 3, 2)
    eng.load_lrts(m, q, pm, thompson_sampling=True)
    eng.set_lrts_block_samples(2)
    got = _update(eng, _fill_store(eng, per), trace=False)
    assert (got[0] > 0).all()
    for a in (0, 1, N // 2, N - 2, N - 1):
        _assert_agent(got, a, oracle.lrts_update(*per[a], m[a], pm[a], q[a]), a)
    eng.close()


def test_workspace_grows_and_is_reused(gpu, oracle):
    """Three updates on one engine at 64 samples per workgroup, each from the previous posterior:
    about 300, then 2400 (the sample workspace and the workgroup tables grow), then 150 samples
    per agent (both reused, larger than needed), against the oracle chained the same way."""
    N, K, Do = 8, 6, 2
    g = np.random.default_rng(53)
    first = [E.ordinary(g, 300 + a, K, Do) for a in range(N)]
    eng, (m, q, pm) = _engine(first, K, Do)
    eng.set_lrts_block_samples(64)
    for round_, base in enumerate((300, 2400, 150)):
        per = {a: _samples(first[a] if round_ == 0 else E.ordinary(g, base + a, K, Do)) for a in range(N)}
        want = [oracle.lrts_update(*per[a], m[a], pm[a], q[a]) for a in range(N)]
        got = _update(eng, _fill_store(eng, per, seed=round_))
        for a in range(N):
            _assert_agent(got, a, want[a], (round_, a))
        m, q, pm = got[2]
    eng.close()


# ------------------------------------------------------------------ C. k_lrts_epoch
def _split(c, cuts):
    """The case's samples cut at `cuts` (ends of all shards but the last)."""
    X, A, y = _samples(c)
    edges = [0, *cuts, len(y)]
    return [(X[lo:hi], A[lo:hi], y[lo:hi]) for lo, hi in zip(edges[:-1], edges[1:])]


def _rp_update(names, K, Do, cuts=None):
    """The per-epoch-launch update of the named cases (one agent each) over len(cuts[0]) + 1 shards:
    engines on the one GPU whose totals slots are summed after every launch, as the multi-GPU
    all-reduce does. The launches end by themselves: within max(oracle epochs) + 2 of them (one
    per epoch, the Laplace sums, the write-back) no agent is training any more. Every shard's
    engine must then hold the oracle's posterior."""
    import torch
    cases = [E.case(n) for n in names]
    shards = 1 if cuts is None else len(cuts[0]) + 1
    pieces = [_split(c, () if cuts is None else cuts[a]) for a, c in enumerate(cases)]
    parts = []
    for r in range(shards):
        eng, _ = _engine(cases, K, Do)
        parts.append((eng, _fill_store(eng, {a: pieces[a][r] for a in range(len(cases))}, seed=r + 1)))
    counts = np.zeros(parts[0][0].N, np.int64)
    counts[:len(cases)] = [len(c["y"]) for c in cases]
    tots = [eng.lrts_rp_begin(st, samples_total=counts) for eng, st in parts]
    bound = max(E.oracle_result(n)[3] for n in names) + 2
    launched, left = 0, len(names)  # (agents without samples are never training)
    while launched < bound and left:
        block = min(256, bound - launched)
        if shards == 1:
            parts[0][0].lrts_rp_epoch(block)
        else:
            for _ in range(block):
                ks = [eng.lrts_rp_epoch(1) for eng, _ in parts]
                s = sum(t[k & 1] for t, k in zip(tots, ks))
                for t, k in zip(tots, ks):
                    t[k & 1].copy_(s)
        launched += block
        torch.cuda.synchronize()
        polls = [eng.lrts_rp_poll() for eng, _ in parts]
        assert len(set(polls)) == 1
        left = polls[0]
    assert left == 0, (names, launched, bound, left)
    for eng, _ in parts:
        got = (eng.lrts_rp_end(), None, eng.lrts_state())
        for a, n in enumerate(names):
            _assert_agent(got, a, E.oracle_result(n), (n, shards))
        eng.close()


@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("name", ["cap_k1", "cap_k2"])
def test_rp_epoch_cap(gpu, oracle, name, shards):
    """The cap in the per-epoch form: after epoch 16383's step the fit goes to its Laplace pass by
    itself, 16384 + 2 launches in all."""
    c = E.case(name)
    assert E.oracle_result(name)[3] == E.MAX_EPOCHS
    _rp_update([name], *c["m"].shape, cuts=None if shards == 1 else [(len(c["y"]) // 2,)])


@pytest.mark.parametrize("shards", [1, 2])
def test_rp_saturated(gpu, oracle, shards):
    names = ("saturated", "n2_same_item", "x64_all")
    cuts = None if shards == 1 else [(130,), (1,), (200,)]  # (the third agent: all on shard 0)
    _rp_update(names, 6, 2, cuts=cuts)


@pytest.mark.parametrize("shards", [1, 2])
def test_rp_three_workgroups_per_agent(gpu, oracle, shards):
    """2 * 2048 + 100 samples of one agent on one rank (three workgroups adding up the agent's
    combining tree without waiting) beside an agent on two; under two shards 4100 / 96 and
    2100 / 48."""
    _rp_update(("rp_k12", "rp_k12_b"), 12, 5, cuts=None if shards == 1 else [(4100,), (2100,)])


def test_rp_two_level_tree(gpu, oracle):
    """34 900 samples on one rank: 18 workgroups, the second level of agent_reduce_nowait's tree."""
    _rp_update(("big_k2",), 2, 2)
