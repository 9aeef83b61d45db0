"""The device generator against its plain statement (tests/gen_reference.py), value by value.

ag_generate, ag_generate_noise, ag_generate_ts_noise_compact and ag_generate_search_grid at
64-bit seeds, across the index carry first + i = 2^32, at P on both sides of slot 12 (where the
slots' streams change ranges) and at Thompson widths with whole blocks, a partial last block and
a single coefficient. u, the participants and the search grids are exact. The normals are the
hardware's log2 / sin / cos against the reference's float64 transform of the same float32
operands, so they are compared within Z_TOL in z.

Z_TOL: the largest |z_gpu - z_ref| measured on an MI355X over the directly stored normals of all
the cases of this module (policy_eps; ctx at scale 1; ts_noise at q = 1) was Z_MEASURED =
4.958e-7 (policy_eps 4.96e-7, ctx 4.04e-7, ts_noise 4.12e-7; half a float32 ulp of the largest
|z| is 2.4e-7 of it); the bound asserted is four times that, 1.98e-6 (other seeds and boxes: the
error depends on the argument, not on the box), and must stay below 1e-3 -- a wrong word, pair
or stream moves almost every draw by O(1). Derived values scale it: ts_noise by 1 / sqrtf(q)
plus one float32 ulp, gamma_raw by sigma and ctx by the scale, plus one float64 ulp each (in
units of z the derived values measured at most 6.4e-7, their own rounding included).
"""
import numpy as np
import pytest

import gen_reference as R
from test_gpu_parity import _GEN_POPS

pytestmark = pytest.mark.gpu

Z_MEASURED = 4.958e-7
Z_TOL = 4 * Z_MEASURED
assert Z_TOL < 1e-3

SEEDS = (0, 0x9E3779B97F4A7C15)
CARRY = (1 << 32) - 150
FIRSTS = (0, CARRY, 5_000_000_000)
B0 = 301  # four full 64-lane tiles and a 45-lane tail

_zerr = {}


def _np(t):
    return t.detach().cpu().numpy()


def _check_normals(what, got, ref, factor=1.0, ulp=0.0, direct=False):
    """|got - ref| <= Z_TOL * factor + ulp everywhere, NaN exactly where the reference has NaN;
    the error in units of z is printed (and, for directly stored normals, kept) before."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    factor = np.broadcast_to(np.asarray(factor, np.float64), ref.shape)
    err = np.where(nan, 0.0, np.abs(got - ref))
    with np.errstate(divide="ignore", invalid="ignore"):
        ez = np.where(factor > 0, err / factor, 0.0)
    worst = float(ez.max()) if ez.size else 0.0
    key = what + ("" if direct else " (derived)")
    _zerr[key] = max(_zerr.get(key, 0.0), worst)
    print(f"zerr {key}: {worst:.3e}  (max so far {_zerr[key]:.3e}, Z_TOL {Z_TOL:.3e})")
    bad = err > Z_TOL * factor + ulp
    assert not bad.any(), (what, int(bad.sum()), float(err.max()), np.argwhere(bad)[:5].tolist())


def _untile(tiles, B):
    """ts_noise tiles [P][T][KDo][64] -> [P][B][KDo] (coefficient c of auction i of slot s at
    [s][i / 64][c][i % 64])."""
    t = _np(tiles)
    P, T, KDo, _ = t.shape
    return t.transpose(0, 1, 3, 2).reshape(P, T * 64, KDo)[:, :B]


# ---- ag_generate -----------------------------------------------------------------------------
def _check_generate(eng, seed, first, B, scale):
    import torch
    inp = eng.alloc_inputs(B)
    eng.generate(seed, first, inp)
    torch.cuda.synchronize()
    idx = R.indices(first, B)
    assert np.array_equal(_np(inp["u"]), R.uniforms(seed, idx)), ("u", seed, first)
    assert np.array_equal(_np(inp["part"]), R.participants(seed, idx, eng.N, eng.P)), ("part", seed, first)
    ref = scale * R.context_normals(seed, idx, eng.E)
    _check_normals("ctx", _np(inp["ctx"]), ref, scale, np.spacing(np.abs(ref)), direct=scale == 1.0)
    return inp


@pytest.mark.parametrize("N,P,E,scale", [(7, 3, 5, 1.0), (40, 40, 16, 1.3), (64, 64, 1, 1.0), (6, 1, 2, 1.0)])
def test_generate_every_value(gpu, N, P, E, scale):
    """Every u, participant and context of ag_generate: an odd E and a half-used pair (5, 1),
    four context blocks (16), P = N (40, 64: every Floyd step collides or not by the words
    alone), both seeds, before, across and beyond the index carry."""
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(N, P, 12, E, 0, 1, scale)
    for seed in SEEDS:
        for first in FIRSTS:
            _check_generate(eng, seed, first, B0, scale)
    eng.close()


def test_generate_second_grid_stride_pass(gpu):
    """B = 2048 * 256 + 65: the full 2048-workgroup grid and a second pass of the grid-stride
    loop (one 64-lane wave and one lane more), across the index carry; all values against the
    vectorised reference."""
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(2, 1, 12, 1, 0, 1, 1.0)
    _check_generate(eng, SEEDS[1], CARRY, 2048 * 256 + 65, 1.0)
    eng.close()


# ---- ag_generate_noise / ag_generate_ts_noise_compact ------------------------------------------
_MIXED_N = 40


def _mixed_engine(P, K, OE, q_one=False, E=5):
    """The mixed population of test_wide_participants_match_oracle: Oracle / LR-TS allocators
    alternate, bidders cycle through the five kinds in pairs."""
    from auctiongym_amd.engine import AuctionEngine
    N = _MIXED_N
    g = np.random.default_rng(1000 + 64 * P + K)
    pop = dict(ak=np.array([i % 2 for i in range(N)], np.int32),
               bk=np.array([(i // 2) % 5 for i in range(N)], np.int32),
               pg=0.5 + 0.5 * g.random(N), gs=0.01 + 0.05 * g.random(N),
               q=(0.5 + 3.0 * g.random((N, K, OE + 1))).astype(np.float32))
    if q_one:
        pop["q"] = np.ones((N, K, OE + 1), np.float32)
    eng = AuctionEngine(N, P, K, E, OE, 0, 1.0)
    eng.set_agent_params(pop["ak"], pop["bk"], pop["pg"], pop["gs"])
    eng.load_lrts(g.normal(0, 1, (N, K, OE + 1)).astype(np.float32), pop["q"], thompson_sampling=True)
    return eng, pop


def _check_noise(eng, pop, seed, first, B):
    import torch
    P, KDo = eng.P, eng.K * (eng.OE + 1)
    inp = eng.alloc_inputs(B)
    assert {"gamma_raw", "policy_eps", "ts_noise"} <= set(inp)
    inp["ts_noise"].fill_(float("nan"))  # every lane < B must be written, zeros included
    eng.generate(seed, first, inp)
    eng.generate_noise(seed, first, inp)
    torch.cuda.synchronize()
    idx = R.indices(first, B)
    part = R.participants(seed, idx, eng.N, P)
    assert np.array_equal(_np(inp["part"]), part)
    tag = f"P={P} KDo={KDo} seed={seed:#x} first={first}"
    _check_normals("policy_eps", _np(inp["policy_eps"]), R.policy_normals(seed, idx, P), direct=True)
    ref = R.gamma_raw(seed, idx, part, pop["bk"], pop["pg"], pop["gs"])
    assert np.array_equal(np.isnan(ref), pop["bk"][part] == 0), tag
    with np.errstate(invalid="ignore"):
        _check_normals("gamma_raw", _np(inp["gamma_raw"]), ref, pop["gs"][part], np.spacing(np.abs(ref)))
    ts, rs, flags = R.ts_noise(seed, idx, part, pop["ak"] == 1, pop["q"])
    dense = _untile(inp["ts_noise"], B)
    assert (dense[~flags] == 0.0).all(), tag  # other agents' pairs: zeros
    direct = bool((pop["q"] == 1.0).all())
    _check_normals("ts_noise", dense, ts, rs, np.spacing(np.abs(ts).astype(np.float32)), direct=direct)
    # the compact layout: the same values at the LR-TS pairs' ranks, nothing else
    cin = {"part": inp["part"], "u": inp["u"]}
    n = eng.compact_ts_noise(seed, first, cin)
    torch.cuda.synchronize()
    assert n == int(flags.sum()), tag
    want_ix = np.where(flags, np.cumsum(flags.ravel()).reshape(flags.shape) - 1, -1)
    ix = _np(cin["ts_noise_index"])
    assert np.array_equal(ix, want_ix), tag
    comp = _np(cin["ts_noise"])  # [ceil(n / 64)][KDo][64]: pair j, coefficient c at [j / 64][c][j % 64]
    assert comp.shape == (max(1, (n + 63) // 64), KDo, 64)
    j = ix[flags]
    got = comp[j >> 6, :, j & 63]
    _check_normals("ts_noise compact", got, ts[flags], rs[flags], np.spacing(np.abs(ts[flags]).astype(np.float32)),
                   direct=direct)
    assert np.array_equal(got, dense[flags]), tag  # and bit for bit the dense layout's
    return inp


@pytest.mark.parametrize("K,OE", [(12, 4), (7, 2), (1, 0)])
@pytest.mark.parametrize("P", [2, 8, 12, 13, 16, 40])
def test_noise_every_value(gpu, P, K, OE):
    """Every policy_eps, gamma_raw (NaN exactly for Truthful slots) and Thompson noise value of
    lanes < B, dense (zeros for other agents' pairs) and compact, in the mixed population:
    P on both sides of slot 12, K (OE + 1) = 60 (whole blocks), 21 (a partial last block) and 1."""
    eng, pop = _mixed_engine(P, K, OE)
    for seed in SEEDS:
        for first in FIRSTS:
            _check_noise(eng, pop, seed, first, B0)
    eng.close()


# ---- ag_generate_search_grid ---------------------------------------------------------------------
def _grid(eng, seed, first, B):
    import torch
    buf = {"u": torch.empty(B, dtype=torch.float64, device=eng.device),
           "gamma_grid": torch.full((eng.P, 128, B), float("nan"), dtype=torch.float64, device=eng.device)}
    eng.generate_search_grid(seed, first, buf)
    torch.cuda.synchronize()
    return _np(buf["gamma_grid"])


@pytest.mark.parametrize("P", [2, 13])
def test_search_grid_exact(gpu, P):
    """All 128 grid points of every slot and auction equal the reference bit for bit."""
    from auctiongym_amd.engine import AuctionEngine
    eng = AuctionEngine(16, P, 12, 5, 4, 0, 1.0)
    for seed in SEEDS:
        for first in FIRSTS:
            assert np.array_equal(_grid(eng, seed, first, 130), R.search_grid(seed, R.indices(first, 130), P))
    eng.close()


# ---- shard invariance ------------------------------------------------------------------------
@pytest.mark.parametrize("split", [149, 151])
def test_shard_invariance_across_the_carry(gpu, split):
    """One call over [first, first + B) equals two calls split at an odd point, bit for bit, for
    the three generators: first = 2^32 - 150, so one half ends just below the carry (149: the
    second starts on index 2^32 - 1) or just above it (151)."""
    import torch
    seed, first, B = SEEDS[1], CARRY, B0
    eng, pop = _mixed_engine(13, 7, 2)

    def noise(f, n):
        inp = eng.alloc_inputs(n)
        eng.generate(seed, f, inp)
        eng.generate_noise(seed, f, inp)
        cin = {"part": inp["part"], "u": inp["u"]}
        eng.compact_ts_noise(seed, f, cin)
        torch.cuda.synchronize()
        ix = _np(cin["ts_noise_index"])
        comp = _np(cin["ts_noise"])
        dense_c = np.zeros((eng.P, n, comp.shape[1]), np.float32)
        dense_c[ix >= 0] = comp[ix[ix >= 0] >> 6, :, ix[ix >= 0] & 63]
        return {"ctx": _np(inp["ctx"]), "part": _np(inp["part"]), "u": _np(inp["u"])[None],
                "gamma_raw": _np(inp["gamma_raw"]), "policy_eps": _np(inp["policy_eps"]),
                "ts_noise": _untile(inp["ts_noise"], n).transpose(0, 2, 1), "compact": dense_c.transpose(0, 2, 1),
                "grid": _grid(eng, seed, f, n).reshape(-1, n)}

    whole, a, b = noise(first, B), noise(first, split), noise(first + split, B - split)
    for k, w in whole.items():
        assert np.array_equal(w, np.concatenate([a[k], b[k]], axis=-1), equal_nan=True), k
    eng.close()


# ---- independence, with no reference for the device's values ---------------------------------------
_INDEPENDENCE_SEED = 0x9E3779B97F4A7C15


def test_no_normal_is_drawn_twice_in_an_auction(gpu):
    """Mixed population, P = 16, q = 1 (ts_noise is z itself): within an auction no float among
    its Thompson normals and policy_eps values occurs twice. A shared (block, stream) -- slot 12's
    Thompson block 0 and slot 0's policy draw before the wide slots moved -- repeats a float in
    every auction whose slot 12 holds an LR-TS agent.
    K (OE + 1) = 4 (one Thompson block per slot: every stream collision of the kinds compared is
    in block 0), B = 65: 48 floats per auction at most, few enough that a seed exists for which
    no two of an auction's reference values lie within 2 Z_TOL plus float32 rounding of each
    other -- checked here -- so that two equal floats on the device cannot be chance."""
    import torch
    P, K, OE, B, first = 16, 1, 3, 65, CARRY
    seed = _INDEPENDENCE_SEED
    eng, pop = _mixed_engine(P, K, OE, q_one=True)
    # the seed qualifies (CPU): no two reference values of an auction are that close
    idx = R.indices(first, B)
    lr = (pop["ak"] == 1)[R.participants(seed, idx, eng.N, P)]
    assert lr[12].any() and lr[0].any()
    zr = np.concatenate([np.where(lr[:, :, None], R.thompson_normals(seed, idx, P, 4), np.nan).transpose(1, 0, 2)
                         .reshape(B, -1), R.policy_normals(seed, idx, P).T], axis=1)  # [B][P * 4 + P]
    gap = np.diff(np.sort(zr, axis=1), axis=1)  # NaN (no draw) sorts last
    assert np.nanmin(gap) > 2 * Z_TOL + 2 * np.spacing(np.float32(8.0)), "pick another seed"
    # the device's own values, and nothing else
    inp = eng.alloc_inputs(B)
    eng.generate(seed, first, inp)
    eng.generate_noise(seed, first, inp)
    torch.cuda.synchronize()
    lr = (pop["ak"] == 1)[_np(inp["part"])]
    z = np.concatenate([np.where(lr[:, :, None], _untile(inp["ts_noise"], B), np.nan).transpose(1, 0, 2).reshape(B, -1),
                        _np(inp["policy_eps"]).T], axis=1)
    for i in range(B):
        v = z[i][~np.isnan(z[i])]
        assert v.size == 4 * int(lr[:, i].sum()) + P
        assert np.unique(v).size == v.size, (i, "a normal occurs twice in one auction")
    _check_noise(eng, pop, seed, first, B)  # and they are the reference's (q = 1: ts_noise is z, measured as such)
    eng.close()


# ---- the limit -------------------------------------------------------------------------------
def test_generators_refuse_more_than_64_slots(gpu):
    """gen_stream has streams for 64 slots: every generator refuses P = 65, loudly."""
    import torch
    from auctiongym_amd.engine import AuctionEngine, _ptr
    eng = AuctionEngine(65, 65, 1, 1, 0, 0, 1.0)
    eng.set_agent_params(np.ones(65, np.int32), np.ones(65, np.int32), np.ones(65), np.full(65, 0.02))
    eng.load_lrts(np.zeros((65, 1, 1), np.float32), np.ones((65, 1, 1), np.float32))
    inp = eng.alloc_inputs(4)
    inp["part"].zero_()
    with pytest.raises(NotImplementedError, match="ag_generate: P > 64"):
        eng.generate(0, 0, inp)
    with pytest.raises(NotImplementedError, match="ag_generate_noise: P > 64"):
        eng.generate_noise(0, 0, inp)
    index = torch.zeros((65, 4), dtype=torch.int32, device=eng.device)
    with pytest.raises(NotImplementedError, match="ag_generate_ts_noise_compact: P > 64"):
        eng._check(eng.L.ag_generate_ts_noise_compact(eng._h, 0, 0, 4, _ptr(inp["part"]), _ptr(index),
                                                      _ptr(inp["ts_noise"]), None), "ag_generate_ts_noise_compact")
    with pytest.raises(NotImplementedError, match="ag_generate_search_grid: P > 64"):
        _grid(eng, 0, 0, 4)
    eng.close()
    eng = AuctionEngine(64, 64, 1, 1, 0, 0, 1.0)  # the widest accepted: the last slots' streams
    first = CARRY + 140
    assert np.array_equal(_grid(eng, SEEDS[1], first, 20), R.search_grid(SEEDS[1], R.indices(first, 20), 64))
    eng.close()


# ---- generate mode at the new edges ----------------------------------------------------------------
@pytest.mark.parametrize("pop,P,B", [("k_oracle", 2, B0), ("sp_truthful_ts", 2, B0), ("mix", 8, B0),
                                     ("k_oracle", 2, 70001), ("mix", 8, 70001)])
def test_generate_mode_at_the_edges(gpu, pop, P, B):
    """ag_simulate_generated == ag_generate (+ ag_generate_noise) + ag_simulate, every output and
    the exact counters, at a seed with a high half and a batch across the index carry: with the
    comparisons above this ties the draws made inside the simulate kernels to the reference."""
    import torch
    from auctiongym_amd.engine import AuctionEngine
    seed, first, K, E, OE = SEEDS[1], CARRY, 12, 5, 4
    g = np.random.default_rng(500 + P)
    if pop == "k_oracle":  # OracleAllocator + TruthfulBidder: k_oracle's generate mode
        N = 6
        eng = AuctionEngine(N, P, K, E, OE, 1, 1.3)
    else:
        N, mech, ak, bk, init = _GEN_POPS[pop]
        ak, bk, init = (np.asarray(v, np.int32) for v in (ak, bk, init))
        eng = AuctionEngine(N, P, K, E, OE, mech, 1.0)
        eng.set_agent_params(ak, bk, 0.5 + 0.5 * g.random(N), 0.01 + 0.05 * g.random(N))
    eng.load_catalog(np.concatenate([g.normal(0, 1, (N, K, E)), -3.0 - g.random((N, K, 1))], axis=2),
                     g.lognormal(0.1, 0.2, (N, K)))
    if pop != "k_oracle":
        eng.load_lrts(g.normal(0, 1, (N, K, OE + 1)).astype(np.float32),
                      (0.5 + 3.0 * g.random((N, K, OE + 1))).astype(np.float32), thompson_sampling=True)
        if (bk >= 2).any():
            eng.set_dr_state(g.normal(0, 0.7, (N, 16)).astype(np.float32), init)
    inp = eng.alloc_inputs(B)
    eng.generate(seed, first, inp)
    if pop != "k_oracle":
        eng.generate_noise(seed, first, inp)
    out, cnt = eng.alloc_outputs(B), eng.new_counters()
    eng.simulate(inp, out, cnt)
    out_g, cnt_g = eng.alloc_outputs(B), eng.new_counters()
    eng.simulate_generated(seed, first, out_g, cnt_g)
    torch.cuda.synchronize()
    for k in out:
        assert np.array_equal(_np(out[k]), _np(out_g[k]), equal_nan=True), k
    assert torch.equal(cnt, cnt_g)
    eng.close()
