"""Replay-mode inputs: the reference's per-round random draws, in its order.

src/Auction.py draws, per round, from the ONE numpy Generator shared by everything
(src/main.py:29): integers(1, max_slots + 1) (:30; consumes nothing when max_slots == 1),
normal(0, embedding_var, E) (:33), choice(N, P, replace=False) (:42), then, after the
bids, binomial(1, CTR[winner]) (:65), which for n = 1 consumes exactly one next_double U.
TruthfulBidder / OracleAllocator draw nothing in between. Drawing U with rng.random()
leaves the Generator in the same state as the reference after every round
(tests/golden/make_golden.py asserts that on every captured round), so a batch of
rounds can be drawn up front and resolved on the GPU.

Populations with shading bidders or Thompson-sampling allocators draw more per round, in
slot order after the participants (src/Agent.py:44-53): a shading bidder in its
uninitialised state draws rng.normal(prev_gamma, gamma_sigma) (src/Bidder.py:51, 177, 354,
461); an LR-TS allocator draws torch.normal(0, 1/sqrt(q)) from torch's own global
generator (src/Models.py:31). draw_round_population makes the same calls in the same order.

(The one exception: numpy's binomial draws nothing when p == 0.0 exactly, i.e. when a
winner's sigmoid underflows to 0, which needs items . ctx < -745.)

With max_slots > 1 the round's n = integers(1, max_slots + 1) matters: allocate returns
min(n, P) winners and binomial(1, CTRs[winners]) consumes one next_double per winner, in rank
order (src/Auction.py:60-65). The *_slots functions keep n and draw those min(n, P) doubles;
the functions above draw the word and one double, which is right for one slot only.
"""
import numpy as np
import torch


def draw_round(rng, num_agents, num_participants, embedding_size, embedding_var, max_slots=1):
    rng.integers(1, max_slots + 1)
    ctx = rng.normal(0, embedding_var, size=embedding_size)
    part = rng.choice(num_agents, num_participants, replace=False)
    u = rng.random()
    return ctx, part, u


def draw_rounds(rng, B, num_agents, num_participants, embedding_size, embedding_var, max_slots=1):
    """B rounds -> SoA host arrays ctx [E][B] float64, part [P][B] int32, u [B] float64."""
    ctx = np.empty((embedding_size, B))
    part = np.empty((num_participants, B), np.int32)
    u = np.empty(B)
    for r in range(B):
        c, p, uu = draw_round(rng, num_agents, num_participants, embedding_size, embedding_var,
                              max_slots)
        ctx[:, r] = c
        part[:, r] = p
        u[r] = uu
    return ctx, part, u


def _draw_slot_uniforms(rng, n, num_participants, max_slots):
    """The doubles rng.binomial(1, CTRs[winners]) consumes: min(n, P), NaN-padded to min(max_slots, P)."""
    rows = min(max_slots, num_participants)
    if rows == 1:  # then n >= 1 = rows: one double, as draw_round's
        return np.array([rng.random()])
    us = np.full(rows, np.nan)
    for k in range(min(n, num_participants)):
        us[k] = rng.random()
    return us


def draw_round_slots(rng, num_agents, num_participants, embedding_size, embedding_var, max_slots):
    """One multi-slot round of an OracleAllocator + TruthfulBidder population: ctx, part, the
    round's slot count n and u_slots [min(max_slots, P)] (NaN where nothing is consumed)."""
    n = int(rng.integers(1, max_slots + 1))
    ctx = rng.normal(0, embedding_var, size=embedding_size)
    part = rng.choice(num_agents, num_participants, replace=False)
    return ctx, part, n, _draw_slot_uniforms(rng, n, num_participants, max_slots)


def draw_rounds_slots(rng, B, num_agents, num_participants, embedding_size, embedding_var, max_slots):
    """B rounds of draw_round_slots -> SoA host arrays ctx [E][B], part [P][B] int32, num_slots
    [B] int32, u_slots [min(max_slots, P)][B]."""
    ctx = np.empty((embedding_size, B))
    part = np.empty((num_participants, B), np.int32)
    ns = np.empty(B, np.int32)
    us = np.empty((min(max_slots, num_participants), B))
    for r in range(B):
        ctx[:, r], part[:, r], ns[r], us[:, r] = draw_round_slots(rng, num_agents, num_participants,
                                                                 embedding_size, embedding_var, max_slots)
    return ctx, part, ns, us


M128 = (1 << 128) - 1
M64 = (1 << 64) - 1


def draw_rounds_native_slots(rng, B, num_agents, num_participants, embedding_size, embedding_var, max_slots,
                             shading=None):
    """draw_rounds_native for multi-slot rounds (ag_replay_draw_slots): B rounds of
    draw_round_slots (with `shading`, of draw_round_population's numpy-only draws too) in C, the
    same numbers and generator state as the Python loop. Returns ctx [E][B], part [P][B], gamma_raw
    [P][B] or None, num_slots [B] int32, u_slots [min(max_slots, P)][B] (NaN where nothing is
    consumed)."""
    ctx, part, _, g, ns, us = _native_draws(rng, B, num_agents, num_participants, embedding_size, embedding_var,
                                            max_slots, shading, None, True)
    return ctx, part, g, ns, us


def draw_rounds_native(rng, B, num_agents, num_participants, embedding_size, embedding_var, max_slots=1,
                       shading=None, out=None):
    """B rounds of draw_round (and, with `shading` [N] of (prev_gamma, gamma_sigma) or None,
    of draw_round_population's numpy-only draws: the shading bidders' Gaussian gammas) in C
    (ag_replay_draw), the same numbers and the same generator state afterwards as the Python
    loop. rng must be a numpy Generator on PCG64. Returns SoA host arrays ctx [E][B], part
    [P][B] int32, u [B] and gamma_raw [P][B] (NaN where nothing is drawn; None without
    shading). `out` may supply the arrays (e.g. pinned host tensors' numpy views)."""
    return _native_draws(rng, B, num_agents, num_participants, embedding_size, embedding_var, max_slots, shading,
                         out, False)[:4]


def _native_draws(rng, B, num_agents, num_participants, embedding_size, embedding_var, max_slots, shading, out, slots):
    """The C call behind draw_rounds_native (slots False: ag_replay_draw) and draw_rounds_native_slots
    (True: ag_replay_draw_slots). Always (ctx, part, u, gamma_raw, num_slots, u_slots); the last two
    are None for one-slot draws."""
    import ctypes

    from . import _lib
    st, c = _pcg_in(rng)
    B, N, P, E = int(B), int(num_agents), int(num_participants), int(embedding_size)
    o = out or {}
    ctx = o.get("ctx") if o.get("ctx") is not None else np.empty((E, B))
    part = o.get("part") if o.get("part") is not None else np.empty((P, B), np.int32)
    u = None if slots else o.get("u") if o.get("u") is not None else np.empty(B)  # slots: u_slots' row 0
    g = None
    sh = pg = gs = None
    if shading is not None:
        g = o.get("gamma_raw") if o.get("gamma_raw") is not None else np.empty((P, B))
        sh = np.array([x is not None for x in shading], np.uint8)
        pg = np.array([x[0] if x is not None else 0.0 for x in shading], np.float64)
        gs = np.array([x[1] if x is not None else 1.0 for x in shading], np.float64)
    for a in (ctx, part, u, g):
        if a is not None and not a.flags.c_contiguous:
            raise ValueError("replay arrays must be C-contiguous")
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    L = _lib.load()
    ns = us = None
    if slots:
        ns = np.empty(B, np.int32)
        us = np.empty((min(int(max_slots), P), B))
        _lib.check(L.ag_replay_draw_slots(ctypes.byref(c), B, N, P, E, float(embedding_var), int(max_slots), ptr(sh),
                                          ptr(pg), ptr(gs), ptr(ctx), ptr(part), ptr(g), ptr(u), ptr(ns), ptr(us)),
                   "ag_replay_draw_slots", L)
    else:
        _lib.check(L.ag_replay_draw(ctypes.byref(c), B, N, P, E, float(embedding_var), int(max_slots), ptr(sh),
                                    ptr(pg), ptr(gs), ptr(ctx), ptr(part), ptr(g), ptr(u)), "ag_replay_draw", L)
    _pcg_out(rng, st, c)
    return ctx, part, u, g, ns, us


def _pcg_in(rng):
    from . import _lib
    st = rng.bit_generator.state
    if st.get("bit_generator") != "PCG64":
        raise NotImplementedError("ag_replay_draw restates numpy's PCG64 only")
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    return st, _lib.AgPcg64State(s >> 64, s & M64, inc >> 64, inc & M64, int(st["has_uint32"]), int(st["uinteger"]))


def _pcg_out(rng, st, c):
    st["state"]["state"] = (int(c.state_hi) << 64) | int(c.state_lo)
    st["state"]["inc"] = (int(c.inc_hi) << 64) | int(c.inc_lo)
    st["has_uint32"] = int(c.has_uint32)
    st["uinteger"] = int(c.uinteger)
    rng.bit_generator.state = st


def draw_rounds_native_population_slots(rng, B, num_agents, num_participants, embedding_size, embedding_var,
                                        shading, ts_models, max_slots, policy=None, search=None, kdo_max=None):
    """draw_rounds_native_population for multi-slot rounds (ag_replay_draw_population_slots):
    its returns, then num_slots [B] int32 and u_slots [min(max_slots, P)][B]; u is row 0."""
    return _native_population_draws(rng, B, num_agents, num_participants, embedding_size, embedding_var,
                                    shading, ts_models, max_slots, policy, search, kdo_max, True)


def draw_rounds_native_population(rng, B, num_agents, num_participants, embedding_size, embedding_var,
                                  shading, ts_models, max_slots=1, policy=None, search=None, kdo_max=None):
    """B rounds of draw_round_population in C (ag_replay_draw_population): numpy's draws and
    torch's (the LR-TS Thompson draws of src/Models.py:31, the fitted policies' rsample draws of
    src/Models.py:87-88 / :160-161) in the same order, with the same numbers, leaving both
    generators (rng and torch's global CPU generator) exactly where the Python loop leaves
    them. Returns ctx [E][B], part [P][B] int32, gamma_raw [P][B] (NaN where nothing is drawn)
    or None, u [B], ts_noise in the kernel's tile layout [P][ceil(B/64)][K*Do][64] or None,
    policy_eps [P][B] float32 or None, gamma_grid [P][128][B] or None. kdo_max: the noise rows'
    width K*Do (default: the largest model's)."""
    return _native_population_draws(rng, B, num_agents, num_participants, embedding_size, embedding_var,
                                    shading, ts_models, max_slots, policy, search, kdo_max, False)[:7]


def _native_population_draws(rng, B, num_agents, num_participants, embedding_size, embedding_var, shading, ts_models,
                             max_slots, policy, search, kdo_max, slots):
    """The C call behind draw_rounds_native_population (slots False: ag_replay_draw_population) and
    draw_rounds_native_population_slots (True: ag_replay_draw_population_slots). Always (ctx, part,
    gamma_raw, u, ts_noise, policy_eps, gamma_grid, num_slots, u_slots); the last two are None for
    one-slot draws."""
    import ctypes

    from . import _lib
    B, N, P, E = int(B), int(num_agents), int(num_participants), int(embedding_size)
    st, c = _pcg_in(rng)
    u8 = lambda flags: None if flags is None or not any(flags) else np.array([bool(x) for x in flags], np.uint8)  # noqa: E731
    sh, ts, pol, sea = u8(None if shading is None else [x is not None for x in shading]), \
        u8(None if ts_models is None else [m is not None for m in ts_models]), u8(policy), u8(search)
    pg = gs = std = None
    KDo = 0
    ctx, part, u = np.empty((E, B)), np.empty((P, B), np.int32), np.empty(B)
    g = noise = eps = grid = None
    if sh is not None:
        pg = np.array([x[0] if x is not None else 0.0 for x in shading], np.float64)
        gs = np.array([x[1] if x is not None else 1.0 for x in shading], np.float64)
        g = np.empty((P, B))
    kdo = None
    if ts is not None:
        # an agent's own K*Do (src/main.py:61,66: per-agent num_items); the noise rows of the
        # largest model's width, an agent's draws in its first K_a*Do coefficients
        kdo = np.array([int(m.q.numel()) if m is not None else 0 for m in ts_models], np.int32)
        KDo = int(kdo_max) if kdo_max else int(kdo.max())
        std = np.zeros((N, KDo), np.float32)
        for a, m in enumerate(ts_models):
            if m is not None:
                std[a, :kdo[a]] = (1.0 / torch.sqrt(m.q)).numpy().ravel()  # as src/Models.py:31 computes it
        noise = np.empty((P, (B + 63) // 64, KDo, 64), np.float32)
    if pol is not None:
        eps = np.empty((P, B), np.float32)
    if sea is not None:
        grid = np.empty((P, 128, B))
    blob = None
    if ts is not None or pol is not None:
        blob = torch.get_rng_state().numpy().copy()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    L = _lib.load()
    args = (ctypes.byref(c), ptr(blob), 0 if blob is None else blob.size, B, N, P, E, float(embedding_var),
            int(max_slots), ptr(sh), ptr(pg), ptr(gs), ptr(ts), ptr(std), KDo, ptr(kdo), ptr(pol), ptr(sea), ptr(ctx),
            ptr(part), ptr(g), ptr(u), ptr(noise), ptr(eps), ptr(grid))
    ns = us = None
    if slots:
        ns = np.empty(B, np.int32)
        us = np.empty((min(int(max_slots), P), B))
        _lib.check(L.ag_replay_draw_population_slots(*args, ptr(ns), ptr(us)), "ag_replay_draw_population_slots", L)
    else:
        _lib.check(L.ag_replay_draw_population(*args), "ag_replay_draw_population", L)
    _pcg_out(rng, st, c)
    if blob is not None:
        torch.set_rng_state(torch.from_numpy(blob))
    return ctx, part, g, u, noise, eps, grid, ns, us


def draw_round_population(rng, num_agents, num_participants, embedding_size, embedding_var,
                          shading, ts_models, max_slots=1, policy=None, search=None, kdo_max=None):
    """One round of a general population. shading[a] = (prev_gamma, gamma_sigma) of a shading
    bidder in its uninitialised state (else None); ts_models[a] = the LR-TS model whose
    Thompson draw the round makes (else None); policy[a] = True for a learning bidder bidding
    from its fitted policy, whose rsample draws one standard normal from torch's generator
    (src/Models.py:87-88 / :160-161, via torch.distributions.Normal.rsample); search[a] = True
    for a ValueLearningBidder bidding by search, which draws rng.uniform(0.1, 1.0, 128) and
    sorts it (src/Bidder.py:184-186). Returns ctx [E], part [P], gamma_raw [P] (NaN where
    nothing is drawn), u, ts_noise [P][K*Do] float32 or None, policy_eps [P] float32 (0
    where nothing is drawn) or None, gamma_grid [P][128] (0 where nothing is drawn) or
    None."""
    _, ctx, part, gamma_raw, noise, eps, grid = _round_population_draws(
        rng, num_agents, num_participants, embedding_size, embedding_var, shading, ts_models, max_slots, policy,
        search, kdo_max)
    return ctx, part, gamma_raw, rng.random(), noise, eps, grid


def draw_round_population_slots(rng, num_agents, num_participants, embedding_size, embedding_var,
                                shading, ts_models, max_slots, policy=None, search=None, kdo_max=None):
    """draw_round_population for a multi-slot round: (ctx, part, gamma_raw, u_slots [min(max_slots,
    P)] (NaN where nothing is consumed), ts_noise, policy_eps, gamma_grid, the round's slot count n)."""
    n, ctx, part, gamma_raw, noise, eps, grid = _round_population_draws(
        rng, num_agents, num_participants, embedding_size, embedding_var, shading, ts_models, max_slots, policy,
        search, kdo_max)
    return ctx, part, gamma_raw, _draw_slot_uniforms(rng, n, num_participants, max_slots), noise, eps, grid, n


def _round_population_draws(rng, num_agents, num_participants, embedding_size, embedding_var, shading, ts_models,
                            max_slots, policy, search, kdo_max):
    """A round's draws up to the participants' (everything before the clicks): (n, ctx, part,
    gamma_raw, ts_noise, policy_eps, gamma_grid)."""
    n = int(rng.integers(1, max_slots + 1))
    ctx = rng.normal(0, embedding_var, size=embedding_size)
    part = rng.choice(num_agents, num_participants, replace=False)
    gamma_raw = np.full(num_participants, np.nan)
    noise = None
    eps = None
    grid = None
    for s, a in enumerate(part):
        m = ts_models[a]
        if m is not None:  # Agent.select_item: the allocator's Thompson draw first
            z = m.sample_noise().numpy().ravel()
            if noise is None:
                noise = np.zeros((num_participants, kdo_max or z.size), np.float32)
            noise[s, :z.size] = z  # an agent with fewer items: its rows first, zeros after
        if policy is not None and policy[a]:  # then the bidder's
            if eps is None:
                eps = np.zeros(num_participants, np.float32)
            eps[s] = torch.empty(1).normal_().item()
            continue
        if search is not None and search[a]:
            if grid is None:
                grid = np.zeros((num_participants, 128))
            gg = rng.uniform(0.1, 1.0, size=128)
            gg.sort()
            grid[s] = gg
            continue
        sh = shading[a]
        if sh is not None:
            gamma_raw[s] = rng.normal(sh[0], sh[1])
    return n, ctx, part, gamma_raw, noise, eps, grid
