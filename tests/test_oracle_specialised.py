"""k_oracle's specialised builds (ag_sim_oracle.h: the output set FM compile-time) against
the builds they stand in for.

The host picks the specialised build for E = 5 and the output set engine.HEADLINE_FIELDS,
whatever K and P, and runs it at its own grid (kOraSpecBlocksPerCu). Every case here runs three arms on the same inputs and
requires that they agree exactly (NaN equal to NaN, the counters' limbs included):
  1. the engine as it dispatches by itself (the specialised build where there is one);
  2. the same engine told to use the general simulate kernel (AG_OPT_SIMULATE_KERNEL);
  3. oracle.simulate on the host.
Output arrays are filled with a byte pattern before every call, so an element a kernel
leaves unwritten cannot agree by chance.
"""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FULL = ("winner", "price", "second_price", "outcome", "item", "bid", "est_ctr", "true_ctr", "best_ev")
PER_SLOT = ("item", "bid", "est_ctr", "true_ctr", "best_ev")
PER_AUCTION = ("winner", "price", "second_price", "outcome")
# a lone lane; the tile edge (64); the chunk edge (64 * kOraChunkTiles = 512); the wrap where
# work counter 0 is claimed a second time (64 counters * 512 = 32768)
SIZES = (1, 63, 64, 65, 511, 512, 513, 32767, 32768, 32769)
FIRST_PRICE, SECOND_PRICE = 0, 1

_catalogues = {}


def _catalogue(K=12):
    """SP_Oracle's catalogue as main.parse_config draws it (bench.catalogue), with K items."""
    if K not in _catalogues:
        import bench
        cfg = copy.deepcopy(bench.SP_ORACLE)
        cfg["agents"][0]["num_items"] = K
        _catalogues[K] = bench.catalogue(cfg)
    return _catalogues[K]


def _headline():
    from auctiongym_amd.engine import HEADLINE_FIELDS
    return HEADLINE_FIELDS


def _engine(items, values, mech, P=2, generic=False, launch=0):
    from auctiongym_amd.engine import AuctionEngine
    N, K, D = items.shape
    eng = AuctionEngine(N, P, K, D - 1, 4, mech, 1.0)
    eng.load_catalog(items, values)
    eng.set_simulate_kernel(generic)
    if launch:
        eng.set_launch_auctions(launch)
    return eng


def _inputs(eng, B):
    import torch
    inp = eng.alloc_inputs(B)
    eng.generate(0, 0, inp)
    torch.cuda.synchronize()
    return inp


def _alloc(eng, B, fields):
    import torch
    out = eng.alloc_outputs(B, fields)
    for t in out.values():
        t.view(torch.uint8).fill_(0xA5)
    return out


def _numpy(out):
    from auctiongym_amd.engine import unpack_outputs
    return {k: v.cpu().numpy() for k, v in unpack_outputs(out).items() if k != "winner_outcome"}


def _run(eng, inp, fields, counters=True):
    import torch
    B = inp["u"].shape[0]
    out = _alloc(eng, B, fields)
    cnt = eng.new_counters() if counters else None
    eng.simulate(inp, out, cnt)
    torch.cuda.synchronize()
    return _numpy(out), (cnt.cpu().numpy() if counters else None)


def _host(oracle, items, values, mech, inp):
    ctx = np.ascontiguousarray(inp["ctx"].cpu().numpy().T)
    part = np.ascontiguousarray(inp["part"].cpu().numpy().T)
    return oracle.simulate(mech, items, values, ctx, part, inp["u"].cpu().numpy())


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _assert_equals_host(o, cnt, orc, what):
    for f in PER_SLOT:
        if f in o:
            assert _same(o[f].T, orc[f]), (what, f)
    for f in PER_AUCTION:
        if f in o:
            assert _same(o[f], orc[f]), (what, f)
    if cnt is not None:
        assert np.array_equal(cnt, orc["counters_fx"]), (what, "counters")


def _three_arms(oracle, items, values, mech, B, P=2, launch=0):
    """Arms 1 and 2 with the headline output set, arm 3 on the host; returns arm 1's and the
    host's results."""
    engs = [_engine(items, values, mech, P, generic, launch) for generic in (False, True)]
    try:
        inp = _inputs(engs[0], B)
        o1, c1 = _run(engs[0], inp, _headline())
        o2, c2 = _run(engs[1], inp, _headline())
        orc = _host(oracle, items, values, mech, inp)
    finally:
        for e in engs:
            e.close()
    assert set(o1) == set(o2)
    for f in o1:
        assert _same(o1[f], o2[f]), ("specialised vs general kernel", f)
    assert np.array_equal(c1, c2), "specialised vs general kernel: counters"
    _assert_equals_host(o1, c1, orc, "specialised vs host")
    _assert_equals_host(o2, c2, orc, "general kernel vs host")
    return o1, orc


@pytest.mark.parametrize("mech", (SECOND_PRICE, FIRST_PRICE), ids=("SecondPrice", "FirstPrice"))
@pytest.mark.parametrize("B", SIZES)
def test_batch_sizes(gpu, oracle, B, mech):
    items, values = _catalogue()
    _three_arms(oracle, items, values, mech, B)


def test_several_launches(gpu, oracle):
    """B = 4097 in launches of 1024: lo > 0 from the second launch on (every stream
    address is rebased on it), and the last launch holds one auction."""
    items, values = _catalogue()
    _three_arms(oracle, items, values, SECOND_PRICE, 4097, launch=1024)


@pytest.mark.parametrize("mech", (SECOND_PRICE, FIRST_PRICE), ids=("SecondPrice", "FirstPrice"))
def test_field_set_dispatch(gpu, oracle, mech):
    """Only the headline set has a specialised build: every other set runs the run-time form,
    and the fields in common are the same."""
    items, values = _catalogue()
    head = tuple(_headline())
    sets = {"headline": head, "full": FULL, "headline + second_price": head + ("second_price",),
            "headline - best_ev": tuple(f for f in head if f != "best_ev")}
    eng = _engine(items, values, mech)
    try:
        inp = _inputs(eng, 513)
        res = {name: _run(eng, inp, fields) for name, fields in sets.items()}
        orc = _host(oracle, items, values, mech, inp)
    finally:
        eng.close()
    o_head, c_head = res["headline"]
    for name, (o, c) in res.items():
        _assert_equals_host(o, c, orc, name)
        assert np.array_equal(c, c_head), name
        for f in set(o) & set(o_head):
            assert _same(o[f], o_head[f]), (name, f)
    assert "second_price" in res["full"][0] and "best_ev" not in res["headline - best_ev"][0]


@pytest.mark.parametrize("K", (11, 10, 13))
def test_item_counts(gpu, oracle, K):
    """The specialised build takes every K (the pair count stays run-time): K = 11, six item
    pairs, one of them half padding; K = 10 and K = 13, five and seven pairs."""
    items, values = _catalogue(K)
    assert items.shape[1] == K
    _three_arms(oracle, items, values, SECOND_PRICE, 513)


@pytest.mark.parametrize("P", (1, 3, 5))
def test_other_participant_counts(gpu, oracle, P):
    """The specialised build exists for every P at E = 5 (P = 1: nobody is charged, the price is
    NaN)."""
    items, values = _catalogue()
    for mech in (SECOND_PRICE, FIRST_PRICE):
        _three_arms(oracle, items, values, mech, 513, P=P)


def test_near_tie_slow_path(gpu, oracle):
    """Each agent has two identical items (2 and 5) and two whose values differ by one ulp
    (1 and 7). Whenever item 2 leads, item 5 ties it in the f32 screen, so the lane takes the
    exact re-scoring path inside the specialised build; the first maximum (item 2) wins."""
    items, values = (a.copy() for a in _catalogue())
    items[:, 5] = items[:, 2]
    values[:, 5] = values[:, 2]
    items[:, 7] = items[:, 1]
    values[:, 7] = np.nextafter(values[:, 1], 10)
    for mech in (SECOND_PRICE, FIRST_PRICE):
        o, orc = _three_arms(oracle, items, values, mech, 513)
        assert (orc["item"] == 2).any(), "no auction chose the duplicated pair: the slow path was not forced"
        assert not (orc["item"] == 5).any()


def test_counters_off(gpu, oracle):
    items, values = _catalogue()
    eng = _engine(items, values, SECOND_PRICE)
    try:
        inp = _inputs(eng, 513)
        o_on, _ = _run(eng, inp, _headline())
        o_off, _ = _run(eng, inp, _headline(), counters=False)
        orc = _host(oracle, items, values, SECOND_PRICE, inp)
    finally:
        eng.close()
    for f in o_on:
        assert _same(o_on[f], o_off[f]), f
    _assert_equals_host(o_off, None, orc, "counters off")


def test_generate_mode(gpu, oracle):
    """simulate_generated (inputs drawn in the kernel; GEN = true has the specialised build
    too) equals generate + simulate, and the host."""
    import torch
    items, values = _catalogue()
    B = 32769
    eng = _engine(items, values, SECOND_PRICE)
    try:
        inp = _inputs(eng, B)
        o_hbm, c_hbm = _run(eng, inp, _headline())
        out = _alloc(eng, B, _headline())
        cnt = eng.new_counters()
        eng.simulate_generated(0, 0, out, cnt)
        torch.cuda.synchronize()
        o_gen, c_gen = _numpy(out), cnt.cpu().numpy()
        orc = _host(oracle, items, values, SECOND_PRICE, inp)
    finally:
        eng.close()
    for f in o_hbm:
        assert _same(o_hbm[f], o_gen[f]), f
    assert np.array_equal(c_hbm, c_gen)
    _assert_equals_host(o_gen, c_gen, orc, "generate mode")


def test_row_offset_guard(gpu):
    """k_oracle forms a ctx row's offset e * B in 32 bits, so ag_simulate refuses a batch whose
    last row would start at or past 2^32: P = 1, E = 5, B = 2^30 + 1 passes B * P < 2^31 and has
    4 * B = 2^32 + 4. The call returns before any launch, so one-element arrays stand in."""
    import ctypes

    import torch
    from auctiongym_amd.engine import _batch_in, _batch_out, _stream
    items, values = _catalogue()
    eng = _engine(items, values, SECOND_PRICE, P=1)
    try:
        inp, out = eng.alloc_inputs(1), eng.alloc_outputs(1, _headline())
        bi, bo = _batch_in(inp), _batch_out(out)
        rc = eng.L.ag_simulate(eng._h, (1 << 30) + 1, ctypes.byref(bi), ctypes.byref(bo), None, _stream())
        msg = eng.L.ag_last_error().decode()
        torch.cuda.synchronize()
    finally:
        eng.close()
    assert rc != 0 and "(D - 2) * B" in msg, (rc, msg)
