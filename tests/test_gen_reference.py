"""The generator's plain statement (tests/gen_reference.py) pinned on the CPU: its Philox
against the oracle's and the Random123 vectors, its uniforms and participants against the
oracle's at 64-bit seeds and across the index carry, its counter table for collisions, and its
normals' distribution and extreme words. tests/test_gpu_generator.py compares the kernels with
it."""
import numpy as np
import pytest

import gen_reference as R

SEEDS = (0, 0x9E3779B97F4A7C15)


def _philox_vec(ctr, key):
    return [int(w) for w in R.philox4x32_10(*ctr, *key)]


def test_philox_matches_random123_vectors_and_oracle(oracle):
    kat = (([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]))
    for ctr, key, want in kat:
        assert _philox_vec(ctr, key) == want
        assert oracle.philox(ctr, key).tolist() == want
    g = np.random.default_rng(2024)
    ctr = g.integers(0, 1 << 32, (10000, 4), dtype=np.uint64)
    key = g.integers(0, 1 << 32, (10000, 2), dtype=np.uint64)
    got = np.stack(R.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[:, 0], key[:, 1]), axis=1)
    want = np.stack([oracle.philox(c, k) for c, k in zip(ctr, key)])
    assert np.array_equal(got, want.astype(np.uint64))


def _edge_indices():
    out = []
    for base in (0, (1 << 32) - 1, 1 << 32, 5_000_000_000):
        out += [base + d for d in (-2, -1, 0, 1, 2, 3) if base + d >= 0]
    return np.array(sorted(set(out)), np.uint64)


def test_oracle_takes_64_bit_seeds(oracle):
    """The seed's high half reaches the oracle's key: seeds that differ only there differ."""
    lo = 0x7F4A7C15
    assert oracle.gen_uniform(lo, 5) != oracle.gen_uniform(lo | (0x9E3779B9 << 32), 5)
    assert oracle.gen_uniform(0, 1 << 32) != oracle.gen_uniform(0, 0)  # and the index's


@pytest.mark.parametrize("N,P", [(7, 3), (40, 40), (64, 64), (6, 1)])
def test_uniforms_and_participants_match_oracle(oracle, N, P):
    idx = _edge_indices()
    for seed in SEEDS:
        u = R.uniforms(seed, idx)
        part = R.participants(seed, idx, N, P)
        assert part.shape == (P, idx.size) and part.dtype == np.int32
        for n, i in enumerate(idx.tolist()):
            assert u[n] == oracle.gen_uniform(seed, i), (seed, i)
            assert np.array_equal(part[:, n], oracle.gen_participants(seed, i, N, P)), (seed, i)
        assert ((part >= 0) & (part < N)).all()
        assert all(len(set(col)) == P for col in part.T.tolist())


def _collisions(calls):
    seen = {}
    for owner, ctr in calls.items():
        seen.setdefault(ctr, []).append(owner)
    return {c: o for c, o in seen.items() if len(o) > 1}


def test_every_counter_has_one_owner():
    """One auction at the widest shape the library accepts (P = 64, K (OE + 1) = 64, E = 16,
    with search grids): every (block, stream) of the table belongs to exactly one draw call --
    no two kinds, slots or blocks share Philox words."""
    calls = R.draw_calls(R.MAX_SLOTS, 64, 16, grids=True)
    assert len(calls) == 1 + 16 + 4 + 64 * (1 + 1 + 16 + 64)
    assert _collisions(calls) == {}
    # and at every narrower P (the table must not depend on P)
    for P in range(1, R.MAX_SLOTS):
        assert _collisions(R.draw_calls(P, 64, 16)) == {}, P


def test_slots_below_twelve_keep_their_streams():
    """Slots 0..11 draw from the streams they always had (4 + s, 16 + s, 32 + s): every batch of
    P <= 12 is the same bits as before the wide slots moved."""
    for s in range(R.WIDE_SLOT):
        assert R.stream("thompson", s) == 4 + s
        assert R.stream("policy", s) == 16 + s
        assert R.stream("grid", s) == 32 + s
    assert [R.stream(k) for k in ("uniform", "picks", "context", "shading")] == [0, 1, 2, 3]


def test_the_old_scheme_collides_from_thirteen_slots():
    """What the collision check is for: with stream = base + slot for every slot (the scheme
    before the wide slots moved), slot 12's Thompson block 0 is slot 0's policy draw, and the
    check reports it from P = 13 up and nothing below."""
    old = dict(R.COUNTER)
    old["thompson"] = lambda slot, coef: (coef // 4, 4 + slot)
    old["policy"] = lambda slot: (0, 16 + slot)
    old["grid"] = lambda slot, point: (point // 2, 32 + slot)
    for P in range(1, 13):
        assert _collisions(R.draw_calls(P, 64, 16, counter=old)) == {}, P
    bad = _collisions(R.draw_calls(13, 64, 16, counter=old))
    assert bad == {(0, 16): [("policy", 0), ("thompson", 12, 0)]}
    assert len(_collisions(R.draw_calls(17, 64, 16, counter=old))) > len(bad)  # policy into grids


def test_reference_normals_are_standard_normal():
    """2e5 counters: mean 0, variance 1, the normal's tail mass (the checks of the trainer's
    synthetic fit noise), for the cos and the sin branch."""
    g = np.random.default_rng(7)
    idx = g.integers(0, 1 << 63, 200_000, dtype=np.uint64)
    w = R._words(SEEDS[1], idx, 3, 5)
    for z in R.box_muller(w[0], w[1]) + R.box_muller(w[2], w[3]):
        assert np.isfinite(z).all()
        assert abs(z.mean()) < 0.01 and abs(z.var() - 1.0) < 0.02
        assert abs(np.mean(np.abs(z) > 1.96) - 0.05) < 0.003
    zc, zs = R.box_muller(w[0], w[1])
    assert abs(np.corrcoef(zc, zs)[0, 1]) < 0.01


def test_box_muller_extreme_words():
    """What csrc/ag_philox.h promises of the transform: a = 0 gives the largest radius, ~6.66;
    a >= 2^32 - 128 rounds u1 to 1, so r = 0; w >= 2^32 - 128 rounds t to 1, so cos = 1 and
    sin = 0; no word gives a NaN or an infinity."""
    top = (1 << 32) - 1
    zc, zs = R.box_muller([0], [0])
    assert abs(zc[0] - np.sqrt(64 * np.log(2.0))) < 1e-12 and 6.66 < zc[0] < 6.67 and zs[0] == 0.0
    a = np.arange(top - 127, top + 1, dtype=np.uint64)
    zc, zs = R.box_muller(a, np.full(a.size, 12345, np.uint64))
    assert (zc == 0.0).all() and (zs == 0.0).all()
    assert R.box_muller([top - 1000], [0])[0][0] > 0.0  # below the rounding range: r > 0
    w = np.arange(top - 127, top + 1, dtype=np.uint64)
    zc, zs = R.box_muller(np.full(w.size, 1 << 31, np.uint64), w)
    r = np.sqrt(-2.0 * np.log(np.float64(np.float32((2.0 ** 31 + 1) * 2.0 ** -32))))
    assert np.array_equal(zc, np.full(w.size, r)) and (np.abs(zs) < 1e-15).all()
    edge = np.array([0, 1, 127, 128, 1 << 31, top - 128, top - 127, top], np.uint64)
    aa, ww = np.meshgrid(edge, edge)
    zc, zs = R.box_muller(aa.ravel(), ww.ravel())
    assert np.isfinite(zc).all() and np.isfinite(zs).all()
    assert max(np.abs(zc).max(), np.abs(zs).max()) <= 6.67


def test_outputs_use_the_table_and_differ_between_slots():
    """The reference's own draws: slots, coefficients and kinds give different values, the seed's
    high half and the index's high word both matter, and 1 / sqrtf(q) is float32."""
    idx = R.indices((1 << 32) - 3, 6)
    assert idx.tolist() == [(1 << 32) - 3 + i for i in range(6)]
    z = R.thompson_normals(SEEDS[1], idx, 16, 21)
    assert len(np.unique(z)) == z.size
    pe = R.policy_normals(SEEDS[1], idx, 16)
    assert len(np.unique(np.concatenate([z.ravel(), pe.ravel()]))) == z.size + pe.size
    assert not np.array_equal(R.policy_normals(SEEDS[1] & 0xFFFFFFFF, idx, 2), pe[:2])
    assert not np.array_equal(R.policy_normals(SEEDS[1], idx - np.uint64(1 << 32), 2), pe[:2])
    g = R.search_grid(0, idx, 2)
    assert g.shape == (2, 128, 6) and (g >= 0.1).all() and (g < 1.0).all() and len(np.unique(g)) == g.size
    rs = R.thompson_rs(np.array([1.0, 2.0, 3.0], np.float32))
    assert rs.dtype == np.float32 and rs[0] == 1.0 and rs[1] == np.float32(1.0) / np.sqrt(np.float32(2.0))
