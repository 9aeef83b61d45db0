"""A plain statement of the device generator (csrc/ag_philox.h, k_generate*), in numpy.

Test helper, not a conftest. Nothing here calls project code: Philox4x32-10 is written out in
uint64 arithmetic, the counter scheme is a table, and the transforms form their operands the
way the kernels do (which float32 roundings happen where) and then evaluate log, sqrt, sin and
cos in float64. The integer outputs (u, the participants, the search grids) are therefore the
kernels' bit for bit; the normals are the exact values the kernels' hardware log2 / sin / cos
approximate.

Counter: (c0, c1) = the global auction index first + i (low, high word), c2 = block,
c3 = stream; key = the seed (low, high word).
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on broadcastable arrays of 32-bit words; returns
    the four output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(v, np.uint64) & _LO for v in (c0, c1, c2, c3, k0, k1)])
    for r in range(10):
        p0 = _M0 * c0  # 32 x 32 -> 64 bits: no overflow in uint64
        p1 = _M1 * c2
        ka = (k0 + np.uint64((_W0 * r) & 0xFFFFFFFF)) & _LO
        kb = (k1 + np.uint64((_W1 * r) & 0xFFFFFFFF)) & _LO
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ ka, p1 & _LO, (p0 >> _S32) ^ c3 ^ kb, p0 & _LO
    return c0, c1, c2, c3


# ---- the counter scheme ---------------------------------------------------------------------
# Slots below WIDE_SLOT keep the streams they always had (4 + s, 16 + s, 32 + s); the slots
# from WIDE_SLOT up, whose old streams ran into the next kind's, have ranges of their own.
MAX_SLOTS = 64
WIDE_SLOT = 12
STREAM = {
    # kind: stream, or (base for slots < WIDE_SLOT, base for the slots from WIDE_SLOT): base + slot
    "uniform": 0,        # block 0: words 0-1 make u, words 2-3 the first two participant picks
    "picks": 1,          # pick step t >= 2: word (t - 2) % 4 of block (t - 2) / 4
    "context": 2,        # Box-Muller pair m (ctx 2m, 2m + 1): words 2 (m % 2), + 1 of block m / 2
    "shading": 3,        # slot s: the first (cos) normal of block s
    "thompson": (4, 64),    # coefficient c of slot s: normal c % 4 of block c / 4
    "policy": (16, 128),    # slot s: the first (cos) normal of block 0
    "grid": (32, 192),      # point j of slot s: 53-bit uniform j % 2 of block j / 2
}


def stream(kind, slot=0):
    st = STREAM[kind]
    if isinstance(st, tuple):
        return st[0 if slot < WIDE_SLOT else 1] + slot
    return st


COUNTER = {
    # kind: (block, stream) of the Philox call that holds the draw
    "uniform": lambda: (0, stream("uniform")),
    "picks": lambda step: ((0, stream("uniform")) if step < 2 else ((step - 2) // 4, stream("picks"))),
    "context": lambda pair: (pair // 2, stream("context")),
    "shading": lambda slot: (slot, stream("shading")),
    "thompson": lambda slot, coef: (coef // 4, stream("thompson", slot)),
    "policy": lambda slot: (0, stream("policy", slot)),
    "grid": lambda slot, point: (point // 2, stream("grid", slot)),
}


def draw_calls(P, KDo, E, grids=True, counter=COUNTER):
    """Every Philox call of one auction as (what it is drawn for, (block, stream)). A call is
    listed once per owner: the uniform and the first two picks share one call by design (its
    four words), as do the four picks, two context pairs, four Thompson coefficients and two
    grid points of one block."""
    calls = {("uniform+picks01",): counter["uniform"]()}
    assert counter["picks"](0) == counter["picks"](1) == counter["uniform"]()
    for step in range(2, P):
        calls[("picks", (step - 2) // 4)] = counter["picks"](step)
    for pair in range((E + 1) // 2):
        calls[("context", pair // 2)] = counter["context"](pair)
    for s in range(P):
        calls[("shading", s)] = counter["shading"](s)
        calls[("policy", s)] = counter["policy"](s)
        for c in range(KDo):
            calls[("thompson", s, c // 4)] = counter["thompson"](s, c)
        if grids:
            for j in range(128):
                calls[("grid", s, j // 2)] = counter["grid"](s, j)
    return calls


# ---- transforms ------------------------------------------------------------------------------
def uniform53(hi, lo):
    """53-bit uniform in [0, 1) from two words."""
    return (((hi << _S32) | lo) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def box_muller(a, w):
    """(z_cos, z_sin) in float64 from the words a, w: u1 = float32((a + 1) 2^-32) in (0, 1],
    t = float32(w) 2^-32 in [0, 1], r = sqrt(-2 ln u1), z = r cos(2 pi t), r sin(2 pi t)."""
    a = np.asarray(a, np.uint64)
    w = np.asarray(w, np.uint64)
    u1 = ((a.astype(np.float64) + 1.0) * 2.0 ** -32).astype(np.float32).astype(np.float64)
    t = (w.astype(np.uint32).astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * t), r * np.sin(2.0 * np.pi * t)


def _words(seed, idx, block, strm):
    seed = int(seed)
    idx = np.asarray(idx, np.uint64)
    return philox4x32_10(idx & _LO, idx >> _S32, block, strm, seed & 0xFFFFFFFF, seed >> 32)


def indices(first, B):
    """The global auction indices first + i as uint64 [B] (wrapping at 2^64 as the kernels do)."""
    return np.uint64(int(first) & (2 ** 64 - 1)) + np.arange(B, dtype=np.uint64)


# ---- reference outputs -----------------------------------------------------------------------
def uniforms(seed, idx):
    w = _words(seed, idx, *COUNTER["uniform"]())
    return uniform53(w[0], w[1])


def participants(seed, idx, N, P):
    """Floyd's sample of P distinct agents of N, slot order = insertion order: int32 [P][B]."""
    idx = np.asarray(idx, np.uint64)
    part = np.empty((P, idx.size), np.int64)
    w = None
    for step in range(P):
        j = N - P + step
        blk, strm = COUNTER["picks"](step)
        if step < 2:
            word = _words(seed, idx, blk, strm)[2 + step]
        else:
            if (step - 2) % 4 == 0:
                w = _words(seed, idx, blk, strm)
            word = w[(step - 2) % 4]
        pick = ((word * np.uint64(j + 1)) >> _S32).astype(np.int64)
        taken = (part[:step] == pick).any(axis=0)
        part[step] = np.where(taken, j, pick)
    return part.astype(np.int32)


def context_normals(seed, idx, E):
    """z of the contexts, float64 [E][B] (ctx = scale * z)."""
    idx = np.asarray(idx, np.uint64)
    z = np.empty((E, idx.size))
    w = None
    for m in range((E + 1) // 2):
        if m % 2 == 0:
            w = _words(seed, idx, *COUNTER["context"](m))
        zc, zs = box_muller(w[2 * (m % 2)], w[2 * (m % 2) + 1])
        z[2 * m] = zc
        if 2 * m + 1 < E:
            z[2 * m + 1] = zs
    return z


def _first_normal(seed, idx, block, strm):
    w = _words(seed, idx, block, strm)
    return box_muller(w[0], w[1])[0]


def policy_normals(seed, idx, P):
    """policy_eps: float64 [P][B]."""
    return np.stack([_first_normal(seed, idx, *COUNTER["policy"](s)) for s in range(P)])


def shading_normals(seed, idx, P):
    return np.stack([_first_normal(seed, idx, *COUNTER["shading"](s)) for s in range(P)])


def gamma_raw(seed, idx, part, bidder_kind, prev_gamma, gamma_sigma, truthful=0):
    """prev_gamma + sigma * z of the slot's agent, NaN for TruthfulBidder slots: [P][B]."""
    z = shading_normals(seed, idx, part.shape[0])
    g = np.asarray(prev_gamma, np.float64)[part] + np.asarray(gamma_sigma, np.float64)[part] * z
    return np.where(np.asarray(bidder_kind)[part] == truthful, np.nan, g)


def thompson_normals(seed, idx, P, KDo):
    """z of every (slot, auction, coefficient): float64 [P][B][KDo]."""
    idx = np.asarray(idx, np.uint64)
    z = np.empty((P, idx.size, KDo))
    for s in range(P):
        for c0 in range(0, KDo, 4):
            w = _words(seed, idx, *COUNTER["thompson"](s, c0))
            four = box_muller(w[0], w[1]) + box_muller(w[2], w[3])
            for t, c in enumerate(range(c0, min(c0 + 4, KDo))):
                z[s, :, c] = four[t]
    return z


def thompson_rs(q):
    """1 / sqrtf(q) as the kernel forms it: float32(1) / sqrt_f32(q), both correctly rounded."""
    return (np.float32(1.0) / np.sqrt(np.asarray(q, np.float32))).astype(np.float32)


def ts_noise(seed, idx, part, lrts, q):
    """Untiled Thompson noise z * rs of the slot's agent, 0 where it is no LR-TS agent:
    (noise float64 [P][B][KDo], rs float64 [P][B][KDo], flags bool [P][B])."""
    N = len(lrts)
    rs = thompson_rs(q).reshape(N, -1).astype(np.float64)[part]
    flags = np.asarray(lrts, bool)[part]
    z = thompson_normals(seed, idx, part.shape[0], rs.shape[2])
    return np.where(flags[:, :, None], z * rs, 0.0), rs, flags


def search_grid(seed, idx, P):
    """U(0.1, 1) grids: float64 [P][128][B], 0.1 + 0.9 u as two rounded operations."""
    idx = np.asarray(idx, np.uint64)
    g = np.empty((P, 128, idx.size))
    for s in range(P):
        for j in range(0, 128, 2):
            w = _words(seed, idx, *COUNTER["grid"](s, j))
            g[s, j] = 0.1 + 0.9 * uniform53(w[0], w[1])
            g[s, j + 1] = 0.1 + 0.9 * uniform53(w[2], w[3])
    return g
