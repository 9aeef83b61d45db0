"""The multi-slot replay draws on the host (ag_replay_draw_slots, ag_replay_draw_population_slots)
against the Python loop that makes the reference's calls and against the reference's own multi-slot
runs (tests/golden/make_golden_slots.py), value for value and generator state for generator state.
No GPU."""
import json

import numpy as np
import pytest
import torch

from slots_cases import SLOT_CAPTURES, capture


def _entered(seed):
    """Two equal generators entered with a buffered 32-bit half (numpy's has_uint32)."""
    a, b = np.random.default_rng(seed), np.random.default_rng(seed)
    a.integers(0, 5), b.integers(0, 5)
    assert a.bit_generator.state["has_uint32"] == 1
    return a, b


@pytest.mark.parametrize("N,P,E,var,slots,seed", [
    (6, 4, 5, 1.0, 3, 0), (6, 2, 5, 1.0, 3, 1), (6, 3, 5, 1.0, 8, 2), (4, 1, 3, 0.5, 2, 3),   # P = 1
    (8, 8, 5, 2.0, 3, 4), (3, 3, 5, 1.0, 8, 5),                                               # P = N, n >= P
    (40, 7, 0, 1.0, 2, 6), (12, 9, 2, 1.0, 8, 7), (6, 2, 5, 1.0, 1, 8)])
def test_native_slot_draws_match_python(N, P, E, var, slots, seed):
    from auctiongym_amd.replay import draw_rounds_native_slots, draw_rounds_slots
    B = 2000
    a, b = _entered(seed)
    ctx, part, g, ns, us = draw_rounds_native_slots(a, B, N, P, E, var, slots)
    c2, p2, n2, u2 = draw_rounds_slots(b, B, N, P, E, var, slots)
    assert g is None
    assert np.array_equal(ctx, c2) and np.array_equal(part, p2) and np.array_equal(ns, n2)
    assert us.shape == (min(slots, P), B) and np.array_equal(us, u2, equal_nan=True)
    assert a.bit_generator.state == b.bit_generator.state and a.random() == b.random()
    assert set(np.unique(ns)) == set(range(1, slots + 1))
    assert np.array_equal(np.isfinite(us).sum(axis=0), np.minimum(ns, P))  # min(n, P) doubles per round
    if slots > P:
        assert (ns >= P).any()


def test_native_slot_draws_with_shading_match_python():
    from auctiongym_amd.replay import draw_round_population_slots, draw_rounds_native_slots
    N, P, E, S, B = 7, 3, 4, 3, 1500
    shading = [(0.9 + 0.01 * a, 0.05) if a % 2 else None for a in range(N)]
    a, b = _entered(11)
    ctx, part, g, ns, us = draw_rounds_native_slots(a, B, N, P, E, 1.0, S, shading)
    for r in range(B):
        c, p, gr, u, _, _, _, n = draw_round_population_slots(b, N, P, E, 1.0, shading, [None] * N, S)
        assert np.array_equal(ctx[:, r], c) and np.array_equal(part[:, r], p) and ns[r] == n
        assert np.array_equal(g[:, r], gr, equal_nan=True) and np.array_equal(us[:, r], u, equal_nan=True)
    assert a.bit_generator.state == b.bit_generator.state


class _TsModel:
    def __init__(self, q):
        self.q = q

    def sample_noise(self):
        return torch.normal(mean=0.0, std=1.0 / torch.sqrt(self.q))


@pytest.mark.parametrize("S,P", [(2, 3), (3, 3), (8, 3), (3, 1)])
def test_native_population_slot_draws_match_python(S, P):
    """torch's draws (Thompson noise, rsample) interleaved with multi-slot numpy draws."""
    from auctiongym_amd.engine import AuctionEngine
    from auctiongym_amd.replay import draw_round_population_slots, draw_rounds_native_population_slots
    N, E, B, KDo = 9, 5, 500, 60
    gen = torch.Generator().manual_seed(5)
    ts = [_TsModel(torch.rand(12, 5, generator=gen) * 3 + 0.05) if a % 3 != 1 else None for a in range(N)]
    policy = [a % 2 == 0 for a in range(N)]
    shading = [(1.0 + 0.1 * a, 0.05) if a % 4 == 1 else None for a in range(N)]
    a, b = _entered(21)
    torch.manual_seed(99)
    t0 = torch.get_rng_state()
    ctx, part, g, u, noise, eps, grid, ns, us = draw_rounds_native_population_slots(a, B, N, P, E, 1.0, shading, ts,
                                                                                   S, policy, None)
    t_native = torch.get_rng_state()
    torch.set_rng_state(t0)
    z = np.zeros((B, P, KDo), np.float32)
    for r in range(B):
        c, p, gr, uu, nz, ee, _, n = draw_round_population_slots(b, N, P, E, 1.0, shading, ts, S, policy, None)
        assert np.array_equal(ctx[:, r], c) and np.array_equal(part[:, r], p) and ns[r] == n
        assert np.array_equal(us[:, r], uu, equal_nan=True) and u[r] == uu[0]
        assert np.array_equal(g[:, r], gr, equal_nan=True)
        assert np.array_equal(eps[:, r], ee if ee is not None else np.zeros(P, np.float32))
        if nz is not None:
            z[r] = nz
    assert torch.equal(torch.get_rng_state(), t_native)
    assert a.bit_generator.state == b.bit_generator.state
    assert np.array_equal(noise, AuctionEngine.tile_ts_noise(z))


@pytest.mark.parametrize("name", SLOT_CAPTURES)
def test_native_slot_draws_reproduce_the_reference(name, tmp_path):
    """From the fixture's config and seed: the reference's slot counts, contexts, participants,
    shading draws and consumed doubles; for the Oracle populations its generator state too."""
    import auctiongym_amd.main as M
    from auctiongym_amd.replay import draw_rounds_native_slots
    d, meta, agg = capture(name)
    p = tmp_path / "cfg.json"
    p.write_text(json.dumps(meta["config"]))
    rng, *_ = M.parse_config(str(p))
    shading = None
    if "Empirical" in meta["bidders"][0]:
        shading = [(kw["init_gamma"], kw["gamma_sigma"]) for kw in meta["bidder_kwargs"]]
    ctx, part, g, ns, us = draw_rounds_native_slots(rng, meta["rounds"], meta["N"], meta["P"], meta["E"], meta["var"],
                                                    meta["max_slots"], shading)
    assert np.array_equal(ns, d["num_slots"]) and np.array_equal(ctx.T, d["ctx"]) and np.array_equal(part.T, d["part"])
    assert np.array_equal(us.T, d["u_slots"], equal_nan=True)
    if shading:
        assert np.array_equal(g.T, d["gamma_raw"], equal_nan=True)
    st = rng.bit_generator.state
    after = agg["rng_state_after"]
    assert (str(st["state"]["state"]), str(st["state"]["inc"]), st["has_uint32"], st["uinteger"]) == \
        (after["state"], after["inc"], after["has_uint32"], after["uinteger"])


@pytest.mark.parametrize("slots", [1, 2, 3, 5])
def test_one_slot_draw_functions_are_unchanged(slots):
    """ag_replay_draw / ag_replay_draw_population share the loop now: they still draw the slots
    word, drop it and consume ONE double, as the Python draw_rounds does."""
    from auctiongym_amd.replay import draw_rounds, draw_rounds_native, draw_rounds_native_population
    N, P, E, B = 8, 3, 5, 1000
    a, b = _entered(31)
    x = draw_rounds_native(a, B, N, P, E, 1.0, slots)
    y = draw_rounds(b, B, N, P, E, 1.0, slots)
    for u, v in zip(x[:3], y):
        assert np.array_equal(u, v)
    assert a.bit_generator.state == b.bit_generator.state
    c, _ = _entered(31)
    ctx, part, g, u, noise, eps, grid = draw_rounds_native_population(c, B, N, P, E, 1.0, None, None, slots)
    assert np.array_equal(ctx, y[0]) and np.array_equal(part, y[1]) and np.array_equal(u, y[2])
    assert c.bit_generator.state == b.bit_generator.state


def _same(x, y):
    if x is None or y is None:
        return x is None and y is None
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("pop", ["plain", "shading", "ts_policy"])
def test_slot_draws_at_one_slot_are_the_one_slot_draws(pop, P):
    """At max_slots = 1 the four *_slots draw functions give their one-slot counterparts' numbers
    (u_slots[0] == u, num_slots == 1) and leave numpy's generator, and torch's, in the same state:
    what lets Auction draw every round, one-slot ones too, through the *_slots functions."""
    from auctiongym_amd import replay as R
    N, E, B = 6, 5, 200
    shading = [None] * N
    ts = [None] * N
    policy = None
    if pop == "shading":
        shading = [(0.9 + 0.01 * a, 0.05) if a % 2 else None for a in range(N)]
    elif pop == "ts_policy":
        gen = torch.Generator().manual_seed(5)
        ts = [_TsModel(torch.rand(12, 5, generator=gen) * 3 + 0.05) if a % 3 != 1 else None for a in range(N)]
        policy = [a % 2 == 0 for a in range(N)]
        shading = [(1.0 + 0.1 * a, 0.05) if a % 4 == 1 else None for a in range(N)]

    def both(one, slots):
        """Run the pair from equal numpy and torch states; both states must end equal."""
        a, b = _entered(41)
        torch.manual_seed(7)
        x = one(a)
        t_one = torch.get_rng_state()
        torch.manual_seed(7)
        y = slots(b)
        assert torch.equal(torch.get_rng_state(), t_one)
        assert a.bit_generator.state == b.bit_generator.state and a.random() == b.random()
        return x, y

    # the per-round Python draws
    def rounds_one(g):
        return [R.draw_round_population(g, N, P, E, 1.0, shading, ts, 1, policy, None) for _ in range(B)]

    def rounds_slots(g):
        return [R.draw_round_population_slots(g, N, P, E, 1.0, shading, ts, 1, policy, None) for _ in range(B)]
    for (ctx, part, gr, u, nz, ee, grid), (c2, p2, g2, us, n2, e2, grid2, n) in zip(*both(rounds_one, rounds_slots)):
        assert n == 1 and us.shape == (1,) and us[0] == u
        assert all(_same(v, w) for v, w in ((ctx, c2), (part, p2), (gr, g2), (nz, n2), (ee, e2), (grid, grid2)))
    # the native population draws
    sh = shading if pop != "plain" else None
    (ctx, part, gr, u, nz, ee, grid), y = both(
        lambda g: R.draw_rounds_native_population(g, B, N, P, E, 1.0, sh, ts, 1, policy, None),
        lambda g: R.draw_rounds_native_population_slots(g, B, N, P, E, 1.0, sh, ts, 1, policy, None))
    assert all(_same(v, w) for v, w in zip((ctx, part, gr, u, nz, ee, grid), y[:7]))
    assert np.array_equal(y[7], np.ones(B, np.int32)) and y[8].shape == (1, B) and np.array_equal(y[8][0], u)
    if pop == "ts_policy":
        return  # the functions below make numpy's draws only
    (ctx, part, u, gr), (c2, p2, g2, ns, us) = both(
        lambda g: R.draw_rounds_native(g, B, N, P, E, 1.0, 1, sh),
        lambda g: R.draw_rounds_native_slots(g, B, N, P, E, 1.0, 1, sh))
    assert _same(ctx, c2) and _same(part, p2) and _same(gr, g2)
    assert np.array_equal(ns, np.ones(B, np.int32)) and us.shape == (1, B) and np.array_equal(us[0], u)
    if pop == "plain":
        for (ctx, part, u), (c2, p2, n, us) in zip(*both(
                lambda g: [R.draw_round(g, N, P, E, 1.0, 1) for _ in range(B)],
                lambda g: [R.draw_round_slots(g, N, P, E, 1.0, 1) for _ in range(B)])):
            assert n == 1 and us.shape == (1,) and us[0] == u and _same(ctx, c2) and _same(part, p2)


def test_slot_draw_errors():
    from auctiongym_amd.replay import draw_rounds_native_slots
    with pytest.raises(ValueError, match="larger sample than population"):
        draw_rounds_native_slots(np.random.default_rng(0), 4, 3, 4, 2, 1.0, 2)
    with pytest.raises(NotImplementedError, match="AG_MAX_SLOTS"):
        draw_rounds_native_slots(np.random.default_rng(0), 4, 3, 2, 2, 1.0, 9)


def test_slots_out_struct_matches_the_c_header(tmp_path):
    """The ctypes mirror of ag_slots_out has the size and field offsets a C compiler gives
    include/auctiongym.h and sets struct_size itself; AG_MAX_SLOTS agrees; the ABI version stays 17."""
    import ctypes
    import os
    import subprocess

    from auctiongym_amd import _lib
    from conftest import ROOT
    cls = _lib.AgSlotsOut
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "auctiongym.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(ag_slots_out));', 'printf("max %d\\n", AG_MAX_SLOTS);',
             'printf("abi %d\\n", AG_ABI_VERSION);']
    lines += [f'printf("{f} %zu\\n", offsetof(ag_slots_out, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                        check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == cls().struct_size
    assert int(got["max"]) == _lib.MAX_SLOTS and int(got["abi"]) == _lib.ABI_VERSION == 17
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
