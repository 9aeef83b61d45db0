"""Every shipped kernel shape against the oracle, bit for bit (needs an MI355X; `-m gpu`).

The rest of the GPU suite runs one catalogue shape (K = 12, E = 5, OE = 4: D = E + 1 = 6, LR-TS
width OE + 1 = 5). This file runs the others. Inputs are made on the host with numpy (fixed seeds,
the catalogue recipe of the other tests) and uploaded, Thompson noise through tile_ts_noise, so
nothing here leans on the device generator; the oracle gets the same host arrays. Every output
field and the exact counter limbs are compared as test_00_configs_gpu._compare does. Batches are
tiny and chosen for tails: B in {1, 255, 2*256+37} for 256-lane builds, 2*1024+37 for 1024-lane
ones, one case per family split into 300-auction launches.

Instantiations reached (csrc/ag_sim_p.hip, ag_lrts.hip, ag_plugin.hip):
  * k_oracle<P, D>: P in 1..8 x D in {2,3,4,5,7,8}, all 48 (D = 6 is the rest of the suite's);
    the same inputs through k_simulate<P, D, PRUNE, 1, kGenOracle> screened and exact, all 96.
  * exact-scan-only Oracle builds k_simulate<P, D, false>: D in {9, 11, 13, 16} at P in {1, 2, 8};
    K in {17, 33} at D in {3, 8}; a non-positive catalogue value at D = 4.
  * the runtime-P kernel k_simulate<0, D, PRUNE, 1, kGenOracle | kGenAll>: P in {9, 17} at
    D in {2, 5, 8}, screened (PRUNE) for both G; its exact build at D = 2 (the P = 9 capture).
  * general populations, runtime LR-TS width: every (D, G, PRUNE, BT) pick_kernel_for returns off
    the shipped shape -- D in 2..8 x {kGenTruthful, kGenAll} x {screened, exact} in 256 lanes and
    kGenAll screened in 1024 lanes, 35 builds, widths {2, 3, 4, 5, 7, 8}. shape_cases.general_build
    restates the dispatch rules; test_general_table_reaches_every_build enumerates the table
    against them (and checks no row would take the shipped-shape build). Left out on purpose: the
    full P x D product of the general builds -- each build is run at one P of {1, 2, 3, 8} (every
    P meets every D and both populations somewhere in the table), and P in {4, 5, 6, 7} of the
    general builds are run at one D each (3, 4, 7, 8); the Oracle builds above run every P in 1..8
    at every D.
  * k_lrts_train<DO>: DO in {1, 2, 3, 7, 8} (with 5 elsewhere: 4 and 6 are left out), one and
    several workgroups per agent; ag_estimate_ctr at widths 2 and 8; the generator at E in {1, 16}
    and noise tiles of K * (OE + 1) = 21 floats.
  * LR-TS populations at K in {32, 33, 40, 63, 64, 65}: torch.sigmoid's vectorised 32-element chunks
    against its scalar tail (ts_ctr_of) and the sgemv blocks against their remainder rows, per-agent
    item counts on both sides of 32; generate mode's refusal of these shapes.

Shapes the library refuses by design are asserted in test_refused_shapes, never skipped.
"""
import numpy as np
import pytest

from conftest import load_capture, mech_code, pop_args
from shape_cases import (GENERAL_CASES, ORACLE_PINNED, ORACLE_UNPINNED, POP_PINNED, POP_UNPINNED, REF_FIELD,
                         UNPINNED_BOUNDS, general_build, general_builds_shipped, within_bound)
from test_00_configs_gpu import _compare

pytestmark = pytest.mark.gpu

_ALL_FIELDS = ("winner", "price", "second_price", "outcome", "item", "bid", "est_ctr", "true_ctr", "best_ev",
               "gamma", "propensity")


# ---------------------------------------------------------------- host-made inputs
def _catalogue(g, N, K, E):
    """The catalogue recipe of the GPU suite: N(0, 1) embeddings, intercept in (-4, -3), lognormal values."""
    items = np.concatenate([g.normal(0, 1, (N, K, E)), -3.0 - g.random((N, K, 1))], axis=2)
    return items, g.lognormal(0.1, 0.2, (N, K))


def _rounds(g, N, P, E, B):
    """Contexts [B][E], P distinct participants per round [B][P], outcome uniforms [B]."""
    ctx = g.normal(0, 1, (B, E))
    part = np.ascontiguousarray(np.argsort(g.random((B, N)), axis=1)[:, :P].astype(np.int32))
    return ctx, part, g.random(B)


def _upload(eng, ctx, part, u, **more):
    """Row-major host inputs -> the engine's SoA device tensors. more: gamma_raw / policy_eps [B][P],
    ts_noise [B][P][K][Do] (tiled here), gamma_grid [B][P][128], or ts_noise_tiles / ts_noise_index
    as they are."""
    import torch
    d = eng.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
    inp = {"ctx": up(ctx.T), "part": up(part.T.astype(np.int32)), "u": up(u)}
    for k in ("gamma_raw", "policy_eps"):
        if more.get(k) is not None:
            inp[k] = up(more[k].T)
    if more.get("ts_noise") is not None:
        inp["ts_noise"] = up(eng.tile_ts_noise(more["ts_noise"]))
    if more.get("ts_noise_tiles") is not None:
        inp["ts_noise"] = up(more["ts_noise_tiles"])
        inp["ts_noise_index"] = up(more["ts_noise_index"])
    if more.get("gamma_grid") is not None:
        inp["gamma_grid"] = up(more["gamma_grid"].transpose(1, 2, 0))
    return inp


def _simulate(eng, inp, B, fields=None):
    import torch
    out = eng.alloc_outputs(B, fields)
    cnt = eng.new_counters()
    eng.simulate(inp, out, cnt)
    torch.cuda.synchronize()
    return out, cnt


def _host(out, cnt):
    """Device outputs -> row-major host arrays ([B][P] / [B]) + the counter limbs."""
    o = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("item", "bid", "est_ctr", "true_ctr", "best_ev", "gamma", "propensity"):
        if k in o:
            o[k] = np.ascontiguousarray(o[k].T)
    o["counters_fx"] = cnt.cpu().numpy()
    return o


def _oracle_engine(N, P, K, E, mech, items, values):
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(N, P, K, E, min(E, 4), mech, 1.0)
    eng.load_catalog(items, values)
    return eng


# ---------------------------------------------------------------- a. k_oracle<P, D>
@pytest.mark.parametrize("D", [2, 3, 4, 5, 7, 8])
def test_oracle_kernels_every_p(gpu, oracle, D):
    """k_oracle<P, D> for P in 1..8, then the same inputs through k_simulate<P, D, true, 1,
    kGenOracle> (AG_SIM_KERNEL_GENERIC) and the exact scan k_simulate<P, D, false, 1, kGenOracle>
    (AG_ITEM_SEARCH_EXACT): all three equal the oracle in every field and counter limb. Mechanisms
    alternate, K cycles through {2, 3, 7, 16} (the screen's odd-K pair tail, its full 8 pairs),
    N == P on the even P, B through the tail sizes; P = 5 runs as two 300-auction launches."""
    E = D - 1
    for P in range(1, 9):
        n = D * 8 + P
        K, mech, B = (2, 3, 7, 16)[n % 4], n % 2, (1, 255, 549)[n % 3]
        N = P if P % 2 == 0 else P + 3
        g = np.random.default_rng(9000 + n)
        items, values = _catalogue(g, N, K, E)
        ctx, part, u = _rounds(g, N, P, E, 549 if P == 5 else B)
        B = len(u)
        orc = oracle.simulate(mech, items, values, ctx, part, u)
        eng = _oracle_engine(N, P, K, E, mech, items, values)
        if P == 5:
            eng.set_launch_auctions(300)
        inp = _upload(eng, ctx, part, u)
        _compare(*_simulate(eng, inp, B), orc, f"k_oracle P={P} D={D} K={K} B={B}")
        eng.set_simulate_kernel(True)
        _compare(*_simulate(eng, inp, B), orc, f"k_simulate screened P={P} D={D} K={K} B={B}")
        eng.set_item_search(True)
        _compare(*_simulate(eng, inp, B), orc, f"k_simulate exact P={P} D={D} K={K} B={B}")
        eng.close()


# ---------------------------------------------------------------- b. exact-scan-only shapes
@pytest.mark.parametrize("D", [9, 11, 13, 16])
def test_exact_scan_wide_embeddings(gpu, oracle, D):
    """E + 1 in {9, 11, 13, 16}: beyond the screen's D <= 8, k_simulate<P, D, false> at P in {1, 2, 8}."""
    E = D - 1
    for i, P in enumerate((1, 2, 8)):
        K, mech, B = (3, 12, 7)[i], (D + i) % 2, (255, 549, 1)[(D + i) % 3]
        N = P + (2, 0, 3)[i]
        g = np.random.default_rng(9500 + D * 10 + P)
        items, values = _catalogue(g, N, K, E)
        ctx, part, u = _rounds(g, N, P, E, B)
        eng = _oracle_engine(N, P, K, E, mech, items, values)
        if P == 2:
            eng.set_launch_auctions(300)
        orc = oracle.simulate(mech, items, values, ctx, part, u)
        _compare(*_simulate(eng, _upload(eng, ctx, part, u), B), orc, f"exact P={P} D={D} K={K} B={B}")
        eng.close()


@pytest.mark.parametrize("K,D,P,mech,B", [(17, 3, 2, 1, 549), (17, 8, 3, 0, 255), (33, 3, 8, 0, 1), (33, 8, 1, 1, 549),
                                          (7, 4, 2, 1, 549)], ids=["K17_D3", "K17_D8", "K33_D3", "K33_D8", "negative"])
def test_exact_scan_large_catalogues_and_negative_value(gpu, oracle, K, D, P, mech, B):
    """More than 16 items (no screen pairs left), and one negative catalogue value at D = 4 (the
    screens rank by 1 / (CTR * value): positive values only) -- the exact scan, equal to the oracle."""
    E, N = D - 1, P + 2
    g = np.random.default_rng(9700 + K * 10 + D)
    items, values = _catalogue(g, N, K, E)
    if K == 7:
        values[1, 4] = -0.75
    ctx, part, u = _rounds(g, N, P, E, B)
    eng = _oracle_engine(N, P, K, E, mech, items, values)
    orc = oracle.simulate(mech, items, values, ctx, part, u)
    out, cnt = _simulate(eng, _upload(eng, ctx, part, u), B)
    _compare(out, cnt, orc, f"exact K={K} D={D} P={P}")
    if K == 7:  # the negative item is chosen by nobody it belongs to
        chosen = out["item"].cpu().numpy().T[part == 1]
        assert chosen.size and (chosen != 4).all()
    eng.close()


# ---------------------------------------------------------------- populations
def _population(pop, N):
    """Plugin kinds, shading parameters and learner states: "ts" LR-TS + TruthfulBidder (kGenTruthful);
    "all" the mix of test_general_kernel_builds_agree -- Oracle / LR-TS allocators x every bidder kind,
    learners uninitialised, bidding from fitted policies (policy_eps) and, for ValueLearningBidders,
    by search over a host grid (kGenAll); "fit" that mix without the search (no [B][P][128] grids)."""
    from auctiongym_amd import _lib
    if pop == "ts":
        return np.ones(N, np.int32), np.zeros(N, np.int32), None, None
    ak = np.array([i % 2 for i in range(N)], np.int32)
    bk = np.array([(i // 2) % 5 for i in range(N)], np.int32)
    init = np.array([1 if bk[a] >= 2 and a % 3 != 1 else 0 for a in range(N)], np.int32)
    modes = np.full(N, _lib.VL_POLICY, np.int32)
    vl = np.flatnonzero(bk == _lib.BIDDER_VALUE_LEARNING) if pop == "all" else []
    for a in vl[::2]:  # every other ValueLearningBidder bids by search
        init[a], modes[a] = _lib.LEARNER_SEARCH, _lib.VL_SEARCH
    return ak, bk, init, modes


def _general_setup(seed, N, P, K, E, OE, mech, pop, sample=True, ragged=False, B=549, catalogue=None, num_items=None):
    """Engine + host inputs + the oracle's answer for a general population of any shape. catalogue:
    (items, values) to use instead of the suite's recipe (the generator's draws stay the same);
    num_items: the agents' own item counts [N] (instead of ragged's random ones)."""
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(seed)
    Do = OE + 1
    items, values = _catalogue(g, N, K, E)
    if catalogue is not None:
        items, values = catalogue
    ak, bk, init, modes = _population(pop, N)
    pg, gs = 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N)
    m = g.normal(0, 1, (N, K, Do)).astype(np.float32)
    q = (1.0 + 3.0 * g.random((N, K, Do))).astype(np.float32)
    state = g.normal(0, 0.7, (N, 16)).astype(np.float32)
    ni = g.integers(1, K + 1, N).astype(np.int32) if ragged else None
    if ragged:
        ni[0] = K
    if num_items is not None:
        ni, ragged = np.asarray(num_items, np.int32), True
    ctx, part, u = _rounds(g, N, P, E, B)
    more = {}
    if sample:
        z = g.normal(0, 1, (B, P, K, Do)) / np.sqrt(q[part])
        more["ts_noise"] = np.where((ak[part] == 1)[:, :, None, None], z, 0.0).astype(np.float32)
    if init is not None:
        more["gamma_raw"] = g.normal(pg[part], gs[part])
        more["policy_eps"] = g.normal(0, 1, (B, P)).astype(np.float32)
        if pop == "all":
            more["gamma_grid"] = g.uniform(0.1, 1.0, (B, P, 128))
    eng = AuctionEngine(N, P, K, E, OE, mech, 1.0)
    eng.set_agent_params(ak, bk, pg, gs)
    if ragged:
        eng.set_agent_items(ni)
    eng.load_catalog(items, values)
    eng.load_lrts(m, q, thompson_sampling=sample)
    if init is not None:
        eng.set_dr_state(state, init)
        eng.set_bidder_modes(modes)
    host = dict(more)  # the oracle's copy: callers may swap the dense noise for the compact layout
    orc = lambda O: O.simulate_pop(mech, items, values, ctx, part, u, ak, bk, pg, gs, OE=OE, ts_m=m,  # noqa: E731
                                   ts_noise=host.get("ts_noise"), gamma_raw=host.get("gamma_raw"), ts_sample=sample,
                                   dr_state=state if init is not None else None, dr_init=init,
                                   policy_eps=host.get("policy_eps"), gamma_grid=host.get("gamma_grid"), num_items=ni)
    return eng, (ctx, part, u, more), orc, dict(ak=ak, bk=bk, m=m, q=q, items=items, values=values)


def _compact(ak, part, noise):
    """The compact Thompson-noise layout of dense host noise [B][P][K][Do]: numpy's exclusive
    cumsum of the LR-TS flags in (slot, auction) order; pair j in tile j // 64, lane j % 64."""
    B, P = part.shape
    flags = (ak[part] == 1).T                                        # [P][B]
    index = np.where(flags, np.cumsum(flags.ravel()).reshape(flags.shape) - 1, -1).astype(np.int32)
    n = int(flags.sum())
    flat = noise.reshape(B, P, -1).transpose(1, 0, 2)[flags]         # [n][K*Do], (slot, auction) order
    tiles = np.zeros((max(1, (n + 63) // 64), flat.shape[1], 64), np.float32)
    j = np.arange(n)
    tiles[j // 64, :, j % 64] = flat
    return index, tiles, n


# ---------------------------------------------------------------- c. the runtime-P kernel
@pytest.mark.parametrize("mixed", [False, True], ids=["oracle", "mixed"])
@pytest.mark.parametrize("P,D", [(9, 2), (9, 5), (9, 8), (17, 2), (17, 5), (17, 8)])
def test_runtime_p_kernel(gpu, oracle, P, D, mixed):
    """More than 8 participants: k_simulate<0, D, true, 1, G> for Oracle-only (kGenOracle) and mixed
    (kGenAll) populations at D in {2, 5, 8}, N == P at P = 17."""
    E = D - 1
    OE = max(1, E - 1)
    N = 17 if P == 17 else 12
    K, mech, B = (3, 7, 16)[(P + D) % 3], (P + D) % 2, (1, 255, 549)[(P // 8 + D // 3) % 3]
    if not mixed:
        g = np.random.default_rng(9900 + P * 10 + D)
        items, values = _catalogue(g, N, K, E)
        ctx, part, u = _rounds(g, N, P, E, B)
        eng = _oracle_engine(N, P, K, E, mech, items, values)
        eng.set_launch_auctions(300 if B == 549 else 0)  # the largest batches as two ragged launches
        orc = oracle.simulate(mech, items, values, ctx, part, u)
        _compare(*_simulate(eng, _upload(eng, ctx, part, u), B), orc, f"runtime-P oracle P={P} D={D} K={K} B={B}")
    else:
        eng, (ctx, part, u, more), orc, _ = _general_setup(9950 + P * 10 + D, N, P, K, E, OE, mech, "all", B=B)
        eng.set_launch_auctions(300 if B == 549 else 0)
        out, cnt = _simulate(eng, _upload(eng, ctx, part, u, **more), B, _ALL_FIELDS)
        _compare(out, cnt, orc(oracle), f"runtime-P mixed P={P} D={D} K={K} B={B}")
    eng.close()


# ---------------------------------------------------------------- d. general populations
def test_general_table_reaches_every_build():
    """The table against the dispatch rules (no GPU needed): every (D, G, PRUNE, BT) build
    pick_kernel_for returns off the shipped shape is launched by at least one row, no row would
    take the shipped-shape build, every P in {1, 2, 3, 8} meets every D and both populations, and
    the axes the issue names are all there."""
    builds = [general_build(c) for c in GENERAL_CASES]
    assert all(b is None or b[1] != "ship" for b in builds)
    assert all(b is not None for b, c in zip(builds, GENERAL_CASES) if c["bt"])  # none of them refused
    assert general_builds_shipped() <= set(builds), general_builds_shipped() - set(builds)
    for P in (1, 2, 3, 8):
        rows = [c for c in GENERAL_CASES if c["P"] == P]
        assert {c["E"] + 1 for c in rows} == set(range(2, 9)), P
        assert {c["pop"] for c in rows} == {"ts", "all"} and {c["mech"] for c in rows} == {0, 1}, P
        assert {c["K"] <= 16 for c in rows} == {True, False}, P
    assert {c["OE"] + 1 for c in GENERAL_CASES} == {2, 3, 4, 5, 7, 8}
    assert {c["K"] for c in GENERAL_CASES} == {3, 7, 12, 16, 17}
    assert {c["bt"] for c in GENERAL_CASES} == {0, 256, 1024}
    assert {(c["pop"], c["sample"]) for c in GENERAL_CASES} == {("ts", True), ("ts", False), ("all", True), ("all", False)}
    assert any(c["ragged"] for c in GENERAL_CASES) and sum(c["compact"] for c in GENERAL_CASES) == 2
    assert {c["bt"] for c in GENERAL_CASES if c["cap"]} == {256, 1024}
    assert {(c["E"], c["OE"]) for c in GENERAL_CASES if c["K"] == 12} == {(5, 3), (4, 4)}


def _case_id(c):
    return "E{E}_OE{OE}_K{K}_P{P}_{pop}_bt{bt}_B{B}".format(**c) + ("_cap" if c["cap"] else "") + \
        ("_ragged" if c["ragged"] else "") + ("_compact" if c["compact"] else "") + ("" if c["sample"] else "_map")


@pytest.mark.parametrize("case", GENERAL_CASES, ids=_case_id)
def test_general_population(gpu, oracle, case):
    """A general population at D != 6 or LR-TS width != 5 (the runtime-width builds of k_simulate;
    shape_cases.GENERAL_CASES): every output and counter limb equal to the oracle on the same host
    inputs -- LR-TS + truthful and the full mix, screened (K in {3, 7, 16}) and exact (K = 17), 256
    and 1024 lanes, Thompson draws and MAP estimates, ragged item counts, dense and compact noise."""
    from auctiongym_amd import _lib
    c = case
    N = 20 if c["pop"] == "all" else 8
    seed = 12000 + GENERAL_CASES.index(c)
    eng, (ctx, part, u, more), orc, pop = _general_setup(seed, N, c["P"], c["K"], c["E"], c["OE"], c["mech"],
                                                         c["pop"], c["sample"], c["ragged"], c["B"])
    if c["bt"]:
        eng._check(eng.L.ag_set_option(eng._h, _lib.OPT_SIM_BLOCK_THREADS, c["bt"]), "ag_set_option")
    eng.set_launch_auctions(c["cap"])
    if c["compact"]:
        index, tiles, n = _compact(pop["ak"], part, more.pop("ts_noise"))
        more.update(ts_noise_tiles=tiles, ts_noise_index=index)
    inp = _upload(eng, ctx, part, u, **more)
    if c["compact"]:  # the library's own index is numpy's
        idx, pairs = eng.ts_noise_index(inp["part"])
        assert pairs == n and np.array_equal(idx.cpu().numpy(), index)
    out, cnt = _simulate(eng, inp, c["B"], _ALL_FIELDS if c["pop"] == "all" else None)
    _compare(out, cnt, orc(oracle), _case_id(c))
    eng.close()


# ---------------------------------------------------------------- a second grid-stride pass
# (path, P, lanes per workgroup): one workgroup per CU and B = CUs * lanes + one full tile + 37, so
# 255 workgroups leave k_simulate's tile loop after one tile while workgroup 0 takes a second, full
# tile and workgroup 1 a ragged one of 37 auctions -- whose idle lanes must leave before the wave
# barriers of the compacted fitted-policy pass -- with counters on.
SECOND_PASS = [("deferred", 2, 256), ("early", 2, 256), ("early_compact", 2, 1024), ("streamed_ts", 3, 256),
               ("streamed_mix", 3, 768), ("runtime_p", 9, 256), ("generate", 3, 256)]


@pytest.mark.parametrize("path,P,lanes", SECOND_PASS, ids=[c[0] for c in SECOND_PASS])
def test_second_grid_stride_pass(gpu, oracle, path, P, lanes):
    """Every tile path of k_simulate over a second grid-stride pass (AG_OPT_SIM_BLOCKS_PER_CU = 1):
    the deferred path (an Oracle population through AG_SIM_KERNEL_GENERIC), the early-count path in
    256 lanes and in 1024 with fitted-policy bidders (the compacted pass), the streamed slots of a
    TruthfulBidder population and of the mix's 768-lane build, and the runtime-P loop -- every output
    and counter limb equal to the oracle's; generate mode's streamed slots against the replay of the
    same draws on the full resident grid."""
    import torch
    from auctiongym_amd import _lib
    from auctiongym_amd.engine import AuctionEngine
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = cus * lanes + lanes + 37
    seed = 13000 + SECOND_PASS.index((path, P, lanes))
    if path == "deferred":
        g = np.random.default_rng(seed)
        N, K, E, mech = 5, 7, 3, 0
        items, values = _catalogue(g, N, K, E)
        ctx, part, u = _rounds(g, N, P, E, B)
        eng = _oracle_engine(N, P, K, E, mech, items, values)
        eng.set_simulate_kernel(True)
        eng.set_blocks_per_cu(1)
        _compare(*_simulate(eng, _upload(eng, ctx, part, u), B), oracle.simulate(mech, items, values, ctx, part, u),
                 f"second pass {path} B={B}")
    elif path == "generate":
        g = np.random.default_rng(seed)
        N, K, E, OE, first = 8, 12, 5, 4, 98765432109
        eng = AuctionEngine(N, P, K, E, OE, 1, 1.0)
        eng.set_agent_params(np.ones(N, np.int32), np.zeros(N, np.int32))
        eng.load_catalog(*_catalogue(g, N, K, E))
        eng.load_lrts(g.normal(0, 1, (N, K, OE + 1)).astype(np.float32),
                      (0.5 + 3.0 * g.random((N, K, OE + 1))).astype(np.float32), thompson_sampling=True)
        inp = eng.alloc_inputs(B)
        eng.generate(11, first, inp)
        eng.generate_noise(11, first, inp)
        out, cnt = _simulate(eng, inp, B)
        eng.set_blocks_per_cu(1)
        out_g, cnt_g = eng.alloc_outputs(B), eng.new_counters()
        eng.simulate_generated(11, first, out_g, cnt_g)
        torch.cuda.synchronize()
        for k in out:
            assert np.array_equal(out[k].cpu().numpy(), out_g[k].cpu().numpy(), equal_nan=True), k
        assert torch.equal(cnt, cnt_g)
    else:
        # (N, K, E, OE, mech, population): the shipped shape where the build is its own (768 lanes)
        N, K, E, OE, mech, pop = {"early": (20, 12, 5, 4, 0, "fit"), "early_compact": (20, 7, 5, 4, 1, "fit"),
                                  "streamed_ts": (8, 12, 5, 4, 1, "ts"), "streamed_mix": (20, 7, 5, 4, 0, "fit"),
                                  "runtime_p": (12, 3, 4, 3, 1, "fit")}[path]
        eng, (ctx, part, u, more), orc, _ = _general_setup(seed, N, P, K, E, OE, mech, pop, B=B)
        if lanes != 768:  # (768 lanes: the library's own choice for the mix at P >= 3)
            eng._check(eng.L.ag_set_option(eng._h, _lib.OPT_SIM_BLOCK_THREADS, lanes), "ag_set_option")
        eng.set_blocks_per_cu(1)
        out, cnt = _simulate(eng, _upload(eng, ctx, part, u, **more), B, _ALL_FIELDS if pop == "fit" else None)
        _compare(out, cnt, orc(oracle), f"second pass {path} B={B}")
    eng.close()


# ---------------------------------------------------------------- e. the reference captures
def _engine_of(meta, d, exact=False):
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(meta["N"], meta["P"], meta["K"], meta["E"], meta["OE"], mech_code(meta), meta["var"])
    eng.set_item_search(exact)
    return eng


@pytest.mark.parametrize("exact", [False, True], ids=["auto", "exact"])
@pytest.mark.parametrize("name", ORACLE_PINNED)
def test_pinned_oracle_captures_replay(gpu, oracle, name, exact):
    """The pinned Oracle captures: every output equal to the reference's, the counters to the
    oracle's, the aggregates to 1e-9 (test_simulate_replay_matches_reference's assertions)."""
    d, meta, agg = load_capture(name)
    eng = _engine_of(meta, d, exact)
    eng.load_catalog(d["items"], d["values"])
    o = _host(*_simulate(eng, _upload(eng, d["ctx"], d["part"], d["u"]), len(d["u"])))
    for mine, ref in (("item", "item"), ("bid", "slot_bid"), ("est_ctr", "slot_est_ctr"),
                      ("true_ctr", "slot_true_ctr"), ("best_ev", "slot_best_ev"), ("winner", "winner"),
                      ("price", "price"), ("second_price", "second_price"), ("outcome", "outcome")):
        assert np.array_equal(o[mine], d[ref]), mine
    orc = oracle.simulate(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"])
    assert np.array_equal(o["counters_fx"], orc["counters_fx"])
    cnt = eng.counters_to_numpy(o["counters_fx"])
    C = {n: i for i, n in enumerate(oracle.COUNTERS)}
    rt = dict(rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(cnt[:, C["net"]], agg["net_utility"], **rt)
    np.testing.assert_allclose(cnt[:, C["gross"]], agg["gross_utility"], **rt)
    np.testing.assert_allclose(cnt[:, C["paid"]].sum(), agg["revenue"], **rt)
    np.testing.assert_allclose(cnt[:, C["underbid_regret"]], agg["underbid_regret"], **rt)
    np.testing.assert_allclose(cnt[:, C["overbid_regret"]], agg["overbid_regret"], **rt)
    eng.close()


def _pop_replay(oracle, name):
    d, meta, _ = load_capture(name)
    args = pop_args(d, meta)
    eng = _engine_of(meta, d)
    eng.set_agent_params(args["alloc_kind"], args["bid_kind"], args["prev_gamma"], args["gamma_sigma"])
    eng.load_catalog(d["items"], d["values"])
    eng.load_lrts(args["ts_m"], np.ones_like(args["ts_m"]), thompson_sampling=True)
    inp = _upload(eng, d["ctx"], d["part"], d["u"], gamma_raw=d["gamma_raw"], ts_noise=d["ts_noise"])
    o = _host(*_simulate(eng, inp, len(d["u"]), _ALL_FIELDS))
    orc = oracle.simulate_pop(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"], **args)
    for k in ("item", "bid", "est_ctr", "true_ctr", "best_ev", "winner", "price", "second_price", "outcome"):
        assert np.array_equal(o[k], orc[k], equal_nan=True), k
    for k in ("gamma", "propensity"):
        real = ~np.isnan(orc[k])
        assert np.array_equal(o[k][real], orc[k][real]), k
    assert np.array_equal(o["counters_fx"], orc["counters_fx"])
    eng.close()
    return d, o


@pytest.mark.parametrize("name", POP_PINNED)
def test_pinned_population_captures_replay(gpu, oracle, name):
    """LR-TS width 5 off the catalogue shape (K = 9, E = 4), truthful and DoublyRobust first
    iteration: equal to the oracle and to the reference itself, float32 CTRs included."""
    d, o = _pop_replay(oracle, name)
    for mine, ref in (("item", "item"), ("winner", "winner"), ("true_ctr", "slot_true_ctr"),
                      ("est_ctr", "slot_est_ctr"), ("bid", "slot_bid"), ("outcome", "outcome")):
        assert np.array_equal(o[mine], d[ref]), mine
    assert np.array_equal(o["price"], d["price"], equal_nan=True)


@pytest.mark.parametrize("name", ORACLE_UNPINNED)
def test_unpinned_oracle_captures_replay(gpu, oracle, name):
    """K = 1 and (D = 8, K = 10): equal to the oracle bit for bit (k_oracle and the exact scan);
    to the reference exactly in item, winner and outcome, in true_ctr within the bound of
    tests/test_oracle_shapes.py (4 x the oracle's own deviation on the fixture)."""
    d, meta, _ = load_capture(name)
    orc = oracle.simulate(mech_code(meta), d["items"], d["values"], d["ctx"], d["part"], d["u"])
    for exact in (False, True):
        eng = _engine_of(meta, d, exact)
        eng.load_catalog(d["items"], d["values"])
        out, cnt = _simulate(eng, _upload(eng, d["ctx"], d["part"], d["u"]), len(d["u"]))
        _compare(out, cnt, orc, f"{name} exact={exact}")
        o = _host(out, cnt)
        for k in ("item", "winner", "outcome"):
            assert np.array_equal(o[k], d[k]), k
        ok, worst = within_bound(o["true_ctr"], d["slot_true_ctr"], UNPINNED_BOUNDS[name]["true_ctr"])
        print(name, "true_ctr relative deviation", worst)
        assert ok, worst
        eng.close()


@pytest.mark.parametrize("name", POP_UNPINNED)
def test_unpinned_lrts_capture_replay(gpu, oracle, name):
    """LR-TS width 3 (E = 3, K = 7): equal to the oracle bit for bit; to the reference exactly in
    item, winner, outcome, true_ctr and best_ev, in est_ctr / bid / price within the bounds of
    tests/test_oracle_shapes.py."""
    d, o = _pop_replay(oracle, name)
    for mine, ref in (("item", "item"), ("winner", "winner"), ("outcome", "outcome"),
                      ("true_ctr", "slot_true_ctr"), ("best_ev", "slot_best_ev")):
        assert np.array_equal(o[mine], d[ref]), mine
    for f, bound in UNPINNED_BOUNDS[name].items():
        ok, worst = within_bound(o[f], d[REF_FIELD[f]], bound)
        print(name, f, "relative deviation", worst)
        assert ok, (f, worst, bound)


# ---------------------------------------------------------------- f. the LR-TS update
def _fill_store(eng, per_agent, seed=0):
    """Caller-owned sample store holding `per_agent` {agent: (X, A, y)}, shuffled."""
    import torch
    key = np.concatenate([(np.int64(a) << 16) | (np.asarray(A, np.int64) << 1) | (np.asarray(y) != 0)
                          for a, (X, A, y) in per_agent.items()]).astype(np.uint32)
    x = np.concatenate([np.asarray(X, np.float32) for X, _, _ in per_agent.values()])
    perm = np.random.default_rng(seed).permutation(len(key))
    key, x = key[perm], x[perm]
    st = eng.new_lrts_samples(len(key))
    st["key"][:] = torch.from_numpy(key.view(np.int32)).to(eng.device)
    st["x"][:] = torch.from_numpy(np.ascontiguousarray(x.T)).to(eng.device)
    st["count"][0] = len(key)
    return st


def _lrts_engine(N, K, Do):
    from auctiongym_amd.engine import AuctionEngine
    E = max(1, Do - 1)
    eng = AuctionEngine(N, 2, K, E, Do - 1, 1, 1.0)
    eng.set_agent_params(np.ones(N, np.int32), np.zeros(N, np.int32))
    return eng


@pytest.mark.parametrize("Do,K", [(1, 5), (2, 32), (3, 7), (7, 9), (8, 8)])
def test_lrts_update_other_widths(gpu, oracle, Do, K):
    """k_lrts_train<DO> at widths other than 5 (K * DO up to 64): three agents -- 300-400 synthetic
    samples for two of them, one sample for the third, which must stay as it is -- against
    oracle.lrts_update: epochs, every epoch's loss, m, q and prev_m bit for bit; then the same
    update split over 64-sample workgroups."""
    g = np.random.default_rng(700 + Do)
    N = 3
    m0 = g.normal(0, 1, (N, K, Do)).astype(np.float32)
    q0 = (1 + g.random((N, K, Do))).astype(np.float32)
    pm0 = (m0 + 0.5).astype(np.float32)
    samples = {}
    for a, n in ((0, 300 + 33 * Do % 100), (1, 1), (2, 400 - Do)):
        X = np.concatenate([g.normal(0, 1, (n, Do - 1)), np.ones((n, 1))], axis=1)
        samples[a] = (X, g.integers(0, K, n), g.random(n) < 0.3)
    eng = _lrts_engine(N, K, Do)
    st = _fill_store(eng, samples)
    want = {a: oracle.lrts_update(*samples[a], m0[a], pm0[a], q0[a]) for a in (0, 2)}
    for chunk in (0, 64):
        eng.set_lrts_block_samples(chunk)
        eng.load_lrts(m0, q0, pm0, thompson_sampling=True)
        ep, tr = eng.lrts_update(st, trace=True)
        m, q, pm = eng.lrts_state()
        tr = tr.cpu().numpy()
        assert ep[1] == 0 and np.array_equal(m[1], m0[1]) and np.array_equal(q[1], q0[1]) and np.array_equal(pm[1], pm0[1])
        for a, (om, opm, oq, oep, oL) in want.items():
            assert oep > 0 and ep[a] == oep, (Do, chunk, a, ep[a], oep)
            assert np.array_equal(tr[a, :oep], oL.astype(np.float32)), (Do, chunk, a)
            assert np.array_equal(m[a], om) and np.array_equal(q[a], oq) and np.array_equal(pm[a], opm), (Do, chunk, a)
    eng.close()


def test_lrts_collect_and_update_width_3(gpu, oracle):
    """An LR-TS + truthful population of E = 3, OE = 2, K = 7 simulated, its won samples collected on
    the GPU (ag_lrts_collect at width 3): the store holds the oracle's winners' samples as a multiset,
    and the update from it equals oracle.lrts_update on them."""
    N, P, K, E, OE, B = 8, 2, 7, 3, 2, 549
    eng, (ctx, part, u, more), orc, pop = _general_setup(777, N, P, K, E, OE, 1, "ts", B=B)
    inp = _upload(eng, ctx, part, u, **more)
    out, cnt = _simulate(eng, inp, B)
    o = orc(oracle)
    _compare(out, cnt, o, "collect width 3")
    st = eng.new_lrts_samples(B)
    eng.lrts_collect(inp, out, st)
    n = int(st["count"][0])
    assert n == B
    key = st["key"][:n].cpu().numpy().view(np.uint32)
    x = st["x"][:, :n].cpu().numpy().T
    r = np.arange(B)
    who, item, y = part[r, o["winner"]], o["item"][r, o["winner"]], o["outcome"]
    X = np.concatenate([ctx[:, :OE], np.ones((B, 1))], axis=1).astype(np.float32)
    want = sorted(zip(((who.astype(np.int64) << 16) | (item.astype(np.int64) << 1) | y).tolist(), map(tuple, X.tolist())))
    assert sorted(zip(key.tolist(), map(tuple, x.tolist()))) == want
    pm0 = (pop["m"] + 0.25).astype(np.float32)
    eng.load_lrts(pop["m"], pop["q"], pm0, thompson_sampling=True)
    ep = eng.lrts_update(st)
    m, q, pm = eng.lrts_state()
    for a in range(N):
        s = who == a
        assert s.sum() >= 2
        om, opm, oq, oep, _ = oracle.lrts_update(X[s], item[s], y[s], pop["m"][a], pm0[a], pop["q"][a])
        assert ep[a] == oep and np.array_equal(m[a], om) and np.array_equal(q[a], oq) and np.array_equal(pm[a], opm), a
    eng.close()


# ---------------------------------------------------------------- g. the per-call surface
@pytest.mark.parametrize("Do", [2, 8])
def test_per_call_lrts_estimate_other_widths(gpu, oracle, Do):
    """PyTorchLogisticRegressionAllocator.estimate_CTR (ag_estimate_ctr) at model widths 2 and 8
    against ora_ts_ctr, shaped like test_per_call_lrts_estimate_matches_oracle_forward: item counts
    with and without a remainder after the sgemv's 4-row blocks, Thompson draw and MAP forward."""
    import torch
    from auctiongym_amd.BidderAllocation import PyTorchLogisticRegressionAllocator
    L = oracle.lib()
    g = np.random.default_rng(80 + Do)
    for K in (1, 3, 4, 7, 8):
        torch.manual_seed(K)
        al = PyTorchLogisticRegressionAllocator(None, Do - 1, K)
        rm = al.response_model
        rm.q = torch.from_numpy(g.uniform(1.0, 400.0, (K, Do)).astype(np.float32))
        for r in range(12):
            x = np.concatenate([g.normal(0, 1, Do - 1), [1.0]])
            x32 = x.astype(np.float32)
            for sample in (True, False):
                state = torch.get_rng_state()
                got = al.estimate_CTR(x, sample=sample)
                torch.set_rng_state(state)
                w = rm.m + torch.normal(mean=0.0, std=1.0 / torch.sqrt(rm.q)) if sample else rm.m
                W = np.ascontiguousarray(w.numpy(), np.float32)
                want = np.array([L.ora_ts_ctr(W[k].ctypes.data, x32.ctypes.data, Do, k, K) for k in range(K)],
                                np.float32)
                assert got.dtype == np.float32 and np.array_equal(got, want), (Do, K, r, sample)


# ---------------------------------------------------------------- h. the device generator
@pytest.mark.parametrize("E", [1, 16])
def test_generator_other_embedding_sizes(gpu, oracle, E):
    """ag_generate at E = 1 and E = 16 (its limit): the uniforms and participants are the oracle's,
    the contexts fill E rows with N(0, var) draws; E = 17 is refused."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    N, P, K, B, first = 7, 3, 4, 301, 5_000_000_000
    eng = AuctionEngine(N, P, K, E, 1, 1, 1.0)
    inp = eng.alloc_inputs(B)
    for t in inp.values():
        t.fill_(-7)
    eng.generate(21, first, inp)
    torch.cuda.synchronize()
    u, part, ctx = inp["u"].cpu().numpy(), inp["part"].cpu().numpy().T, inp["ctx"].cpu().numpy()
    assert np.array_equal(u, np.array([oracle.gen_uniform(21, first + i) for i in range(B)]))
    assert np.array_equal(part, np.stack([oracle.gen_participants(21, first + i, N, P) for i in range(B)]))
    assert ctx.shape == (E, B) and np.isfinite(ctx).all() and (ctx != -7).all()
    n = ctx.size  # N(0, 1): mean within 5 standard errors, variance too (var of z^2 is 2)
    assert abs(ctx.mean()) < 5 / np.sqrt(n) and abs(ctx.var() - 1) < 5 * np.sqrt(2 / n)
    assert len(np.unique(ctx)) == n
    eng.close()
    if E == 16:
        eng = AuctionEngine(N, P, K, 17, 1, 1, 1.0)
        with pytest.raises(NotImplementedError, match="ag_generate: E > 16"):
            eng.generate(21, 0, eng.alloc_inputs(8))
        eng.close()


def test_generated_noise_tiles_and_moments(gpu):
    """ag_generate_noise at (K, OE) = (7, 2) -- tiles of 21 floats: the tiles round-trip through
    untile_ts_noise / tile_ts_noise; the untiled Thompson noise has mean 0 and variance 1 / q per
    coefficient and policy_eps mean 0 and variance 1, each within 5 standard errors of
    its sample size (840k Thompson draws, 262k policy draws)."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    N, P, K, E, OE, B = 6, 2, 7, 3, 2, 20000
    Do = OE + 1
    g = np.random.default_rng(55)
    eng = AuctionEngine(N, P, K, E, OE, 0, 1.0)
    eng.set_agent_params(np.ones(N, np.int32), np.full(N, 4, np.int32), np.ones(N), np.full(N, 0.02))
    q = (0.5 + 3.0 * g.random((N, K, Do))).astype(np.float32)
    eng.load_lrts(g.normal(0, 1, (N, K, Do)).astype(np.float32), q, thompson_sampling=True)
    inp = eng.alloc_inputs(B)
    assert inp["ts_noise"].shape == (P, (B + 63) // 64, K * Do, 64)
    eng.generate(8, 0, inp)
    eng.generate_noise(8, 0, inp)
    torch.cuda.synchronize()
    tiles = inp["ts_noise"].cpu().numpy()
    un = eng.untile_ts_noise(tiles, B)
    assert un.shape == (B, P, K * Do)
    again = eng.tile_ts_noise(un)
    T = B // 64  # whole tiles: identical; the last, partial one up to its B % 64 lanes
    assert again.shape == tiles.shape and np.array_equal(again[:, :T], tiles[:, :T])
    assert np.array_equal(again[:, T, :, :B % 64], tiles[:, T, :, :B % 64])
    assert np.array_equal(eng.untile_ts_noise(again, B), un)
    part = inp["part"].cpu().numpy().T
    z = un.reshape(B, P, K, Do).astype(np.float64) * np.sqrt(q.astype(np.float64))[part]
    n = z.size
    assert n >= 200_000 and abs(z.mean()) < 5 / np.sqrt(n) and abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    for a in range(N):  # per coefficient: variance 1 / q[a, k, j]
        za = un.reshape(B, P, K, Do)[part == a].astype(np.float64)
        na = len(za)
        sd = 1 / np.sqrt(q[a].astype(np.float64))
        assert (np.abs(za.mean(axis=0)) < 5 * sd / np.sqrt(na)).all(), a
        assert (np.abs(za.var(axis=0) * q[a] - 1) < 5 * np.sqrt(2 / na)).all(), a
    Bp = 1 << 17
    big = {"part": torch.empty((P, Bp), dtype=torch.int32, device=eng.device),
           "ctx": torch.empty((E, Bp), dtype=torch.float64, device=eng.device),
           "u": torch.empty((Bp,), dtype=torch.float64, device=eng.device),
           "policy_eps": torch.empty((P, Bp), dtype=torch.float32, device=eng.device)}
    eng.generate(8, 0, big)
    eng.generate_noise(8, 0, big)
    torch.cuda.synchronize()
    pe = big["policy_eps"].cpu().numpy().astype(np.float64)
    n = pe.size
    assert n >= 200_000 and abs(pe.mean()) < 5 / np.sqrt(n) and abs(pe.var() - 1) < 5 * np.sqrt(2 / n)
    eng.close()


# ---------------------------------------------------------------- LR-TS agents with 32 and more items
# torch.sigmoid runs whole 32-element chunks of the K CTRs through its vectorised exp and the rest
# through the scalar one (ts_ctr_of: k < (K & ~31) torch_expf, else expf_glibc), and the Do = 5 logits
# change order at K & ~3: K in {32, 33, 40, 64, 65} puts items on both sides of both splits, K = 63
# has its chunk split (32) away from every other multiple of 16. (K, OE, Thompson sampling, per-agent
# item counts or None, seed): the seeds are ones at which the oracle's choices land on both sides of
# every split the case has (asserted below, so a change of the recipe cannot quietly lose that)
WIDE_LRTS = [(32, 4, True, None, 14000), (33, 4, True, None, 14010), (40, 4, True, None, 14020),
             (64, 4, True, None, 14030), (65, 4, True, None, 14043), (63, 4, True, None, 14050),
             (40, 2, True, None, 14060), (33, 4, False, None, 14070), (64, 4, False, None, 14080),
             (40, 4, True, (31, 32, 33, 40), 14096), (40, 4, False, (31, 32, 33, 40), 14131)]
WIDE_LRTS_MAX_K = 65  # the largest LR-TS catalogue the suite runs (PARITY.md)


@pytest.mark.parametrize("K,OE,sample,counts,seed", WIDE_LRTS,
                         ids=[f"K{c[0]}_OE{c[1]}" + ("" if c[2] else "_map") + ("_counts" if c[3] else "") for c in WIDE_LRTS])
def test_lrts_catalogues_of_32_and_more_items(gpu, oracle, K, OE, sample, counts, seed):
    """LR-TS allocators with truthful bidders (N = 4, P = 2, E = 5, B = 2 * 256 + 37) at K >= 32: the
    vectorised-chunk / scalar split of the CTRs' exp and the sgemv block / remainder split of the
    logits (OE = 4; OE = 2 sums in order), with Thompson draws and as MAP estimates, and with the
    agents' own item counts (31, 32, 33, 40) inside K = 40 -- the splits follow the agent's count,
    not K. Every output and the exact counter limbs equal the oracle's, under the library's own
    kernel choice and under AG_SIM_KERNEL_GENERIC."""
    assert max(c[0] for c in WIDE_LRTS) == WIDE_LRTS_MAX_K
    B = 2 * 256 + 37
    eng, (ctx, part, u, more), orc, _ = _general_setup(seed, 4, 2, K, 5, OE, K % 2, "ts", sample, B=B, num_items=counts)
    want = orc(oracle)
    it = want["item"]
    if counts:  # every agent stays inside its own count; the agent of 33 items chooses its one scalar-path item
        assert (it < np.asarray(counts)[part]).all()
        assert (it[part == 2] == 32).any() and (it[part == 3] >= 32).any() and (it[part == 0] >= 28).any()
    elif K & 31:  # items on both sides of the chunk split (and of the sgemv remainder, where K has one) are chosen
        assert (it >= (K & ~31)).sum() >= 5 and (it < (K & ~31)).any() and (K % 4 == 0 or (it >= (K & ~3)).sum() >= 5)
    inp = _upload(eng, ctx, part, u, **more)
    _compare(*_simulate(eng, inp, B), want, f"LR-TS K={K} OE={OE} sample={sample} counts={counts} auto")
    eng.set_simulate_kernel(True)
    _compare(*_simulate(eng, inp, B), want, f"LR-TS K={K} OE={OE} sample={sample} counts={counts} generic")
    eng.close()


@pytest.mark.parametrize("K", [32, 33, 40, 64, 65])
def test_generate_mode_refuses_32_and_more_items(gpu, K):
    """Generate mode builds the shipped shape's screened item search alone (K <= 16): an LR-TS
    population at K >= 32 is refused, with the limit in the message, not run some other way."""
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(14100 + K)
    eng = AuctionEngine(4, 2, K, 5, 4, 1, 1.0)
    eng.set_agent_params(np.ones(4, np.int32), np.zeros(4, np.int32))
    eng.load_catalog(*_catalogue(g, 4, K, 5))
    eng.load_lrts(g.normal(0, 1, (4, K, 5)).astype(np.float32), np.ones((4, K, 5), np.float32))
    with pytest.raises(NotImplementedError, match=r"ag_simulate_generated: general populations in the shipped shape "
                                                  r"only \(E = 5, OE = 4, K <= 16, .*P=2 D=6\)"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(64))
    eng.close()


# ---------------------------------------------------------------- shapes refused by design
def test_refused_shapes(gpu):
    """What the library does not build is refused loudly, with the limit in the message:
      * E + 1 = 10 (the exact scan builds D in {2..9, 11, 13, 16});
      * E + 1 = 9 with P = 9 (the runtime-P kernel stops at D = 8);
      * a general population with E + 1 > 8;
      * 1024-lane workgroups without the screened item search (K = 17) or with P > 8;
      * generate mode off the shipped shape: a general population at E = 3, one with P = 9, one whose
        LDS image does not fit, an Oracle population at D = 9;
      * the LR-TS trainer at K * (OE + 1) = 65; width 9 cannot be set up at all (E + 1 > 8);
      * ag_generate beyond E = 16 (test_generator_other_embedding_sizes)."""
    from auctiongym_amd import _lib
    from auctiongym_amd.engine import AuctionEngine
    g = np.random.default_rng(6)

    def oracle_engine(N, P, K, E):
        eng = AuctionEngine(N, P, K, E, 4, 1, 1.0)
        eng.load_catalog(*_catalogue(g, N, K, E))
        return eng

    def general_engine(N, P, K, E, OE):
        eng = AuctionEngine(N, P, K, E, OE, 0, 1.0)
        eng.set_agent_params(np.ones(N, np.int32), np.zeros(N, np.int32))
        eng.load_catalog(*_catalogue(g, N, K, E))
        eng.load_lrts(g.normal(0, 1, (N, K, OE + 1)).astype(np.float32), np.ones((N, K, OE + 1), np.float32))
        return eng

    def run(eng, B=64):
        N, P, K, E = eng.N, eng.P, eng.K, eng.E
        ctx, part, u = _rounds(g, N, P, E, B)
        more = {"ts_noise": np.zeros((B, P, K, eng.OE + 1), np.float32)} if getattr(eng, "lrts", False) else {}
        eng.simulate(_upload(eng, ctx, part, u, **more), eng.alloc_outputs(B))

    eng = oracle_engine(4, 2, 5, 9)
    with pytest.raises(NotImplementedError, match=r"E\+1 in \{2\.\.9,11,13,16\}.*D=10"):
        run(eng)
    eng.close()
    eng = oracle_engine(10, 9, 5, 8)
    with pytest.raises(NotImplementedError, match=r"E\+1 <= 8 when P > 8.*P=9, D=9"):
        run(eng)
    eng.close()
    eng = AuctionEngine(4, 2, 5, 8, 4, 0, 1.0)
    with pytest.raises(NotImplementedError, match=r"general populations support E\+1 <= 8 \(D=9\)"):
        eng.set_agent_params(np.ones(4, np.int32), np.zeros(4, np.int32))
    eng.close()
    for N, P, K in ((4, 2, 17), (10, 9, 7)):
        eng = general_engine(N, P, K, 3, 2)
        eng._check(eng.L.ag_set_option(eng._h, _lib.OPT_SIM_BLOCK_THREADS, 1024), "ag_set_option")
        with pytest.raises(NotImplementedError, match=r"AG_OPT_SIM_BLOCK_THREADS = 1024 needs the screened item "
                                                      r"search \(K <= 16.*P <= 8"):
            run(eng)
        eng.close()
    eng = general_engine(4, 2, 7, 3, 2)
    with pytest.raises(NotImplementedError, match=r"shipped shape only \(E = 5, OE = 4"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(64))
    eng.close()
    eng = general_engine(10, 9, 12, 5, 4)
    with pytest.raises(NotImplementedError, match=r"ag_simulate_generated: general populations need P <= 8 \(P=9\)"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(64))
    eng.close()
    eng = general_engine(400, 2, 12, 5, 4)  # 400 x 12 x 6 doubles of catalogue alone: 225 KiB > the 160 KiB of LDS
    with pytest.raises(NotImplementedError, match=r"ag_simulate_generated: supports .* catalogue that fits LDS"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(64))
    with pytest.raises(NotImplementedError, match=r"ag_simulate: supports .* catalogue that fits LDS"):
        run(eng)
    eng.close()
    eng = oracle_engine(4, 2, 5, 8)
    with pytest.raises(NotImplementedError, match=r"ag_simulate_generated: .*E \+ 1 <= 8"):
        eng.simulate_generated(0, 0, eng.alloc_outputs(64))
    eng.close()
    # the LR-TS trainer: K * (OE + 1) = 65 columns do not fit its 64-column accumulator tile
    eng = _lrts_engine(2, 13, 5)
    eng.load_lrts(np.zeros((2, 13, 5), np.float32), np.ones((2, 13, 5), np.float32))
    X = np.concatenate([g.normal(0, 1, (10, 4)), np.ones((10, 1))], axis=1)
    st = _fill_store(eng, {0: (X, g.integers(0, 13, 10), g.random(10) < 0.5)})
    with pytest.raises(NotImplementedError, match=r"ag_lrts_update: needs OE\+1 <= 8 and K\*\(OE\+1\) <= 64 \(K=13, OE\+1=5\)"):
        eng.lrts_update(st)
    eng.close()
    eng = AuctionEngine(2, 2, 4, 8, 8, 1, 1.0)  # width 9 needs OE = 8 <= E: D = 9, no LR-TS population
    with pytest.raises(NotImplementedError, match=r"general populations support E\+1 <= 8 \(D=9\)"):
        eng.set_agent_params(np.ones(2, np.int32), np.zeros(2, np.int32))
    eng.close()
