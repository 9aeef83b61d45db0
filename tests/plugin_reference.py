"""The per-call plugin surface (ag_estimate_ctr, ag_bid), stated with the oracle's own scalars.

One plugin of one agent answers n requests; each answer is the scalar the oracle's batched replay
(oracle/ag_oracle.c simulate_range) computes for the same participant, called once per request
(and item) in a Python loop -- no arithmetic of the project's, no GPU:

    oracle_ctr   OracleAllocator.estimate_CTR         ora_sigmoid(ora_dot(item, x))
    lrts_ctr     PyTorchLogisticRegressionAllocator   ora_ts_ctr(m [+ noise], float32(x), k, K)
    bid          Bidder.bid of every kind and state   ora_propensity / ora_policy_bid / ora_search_gamma

and, apart from the oracle, oracle_ctr_longdouble: the same CTR as plain numpy in np.longdouble
(products summed in order, then 1 / (1 + exp(-z))), with oracle_ctr_bound, the distance a correctly
rounded double evaluation may keep from it.

Codes are those of include/auctiongym.h (AG_BIDDER_*, AG_LEARNER_*). A learner's state16 row is its
win-rate model (w0 w1 w2 b) followed by the 12 parameters of its policy.
"""
import ctypes

import numpy as np

import oracle as O

TRUTHFUL, EMPIRICAL_SHADED, VALUE_LEARNING, POLICY_LEARNING, DOUBLY_ROBUST = range(5)
UNINITIALISED, POLICY, SEARCH = range(3)
ALLOCATOR_ORACLE, ALLOCATOR_LRTS = 0, 1
GRID_POINTS = 128

_bound = False


def lib():
    """The oracle's library with every scalar used here bound (oracle.py binds some of them)."""
    global _bound
    L = O.lib()
    if not _bound:
        d, f, i32, i64, vp = ctypes.c_double, ctypes.c_float, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
        L.ora_dot.restype, L.ora_dot.argtypes = d, [vp, vp, i32]
        L.ora_sigmoid.restype, L.ora_sigmoid.argtypes = d, [d]
        L.ora_ts_ctr.restype, L.ora_ts_ctr.argtypes = f, [vp, vp, i32, i32, i32]
        L.ora_propensity.restype, L.ora_propensity.argtypes = d, [d, d, d]
        L.ora_policy_bid.restype, L.ora_policy_bid.argtypes = None, [vp, d, d, f, vp, vp]
        L.ora_search_gamma.restype, L.ora_search_gamma.argtypes = d, [vp, d, d, vp, i64]
        _bound = True
    return L


def oracle_ctr(items, x):
    """items [K][D], x [n][D] (the true context with its intercept) -> float64 [n][K]."""
    L = lib()
    items = np.ascontiguousarray(items, np.float64)
    x = np.ascontiguousarray(x, np.float64)
    (K, D), n = items.shape, x.shape[0]
    assert x.shape == (n, D)
    out = np.empty((n, K))
    ip, xp = items.ctypes.data, x.ctypes.data
    for i in range(n):
        for k in range(K):
            out[i, k] = L.ora_sigmoid(L.ora_dot(ip + 8 * D * k, xp + 8 * D * i, D))
    return out


def lrts_ctr(m, x, noise=None):
    """m [K][Do] float32, x [n][Do] (the observed context with its intercept, rounded to float32
    as the reference's torch.from_numpy(context.astype(float32))), noise [n][K][Do] float32 Thompson
    draws or None (the MAP forward). w = m + noise in float32; float32 CTRs widened to float64
    [n][K]."""
    L = lib()
    m = np.ascontiguousarray(m, np.float32)
    x32 = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32))
    (K, Do), n = m.shape, x32.shape[0]
    assert x32.shape == (n, Do)
    if noise is None:
        w = np.ascontiguousarray(np.broadcast_to(m, (n, K, Do)))
    else:
        noise = np.asarray(noise, np.float32)
        assert noise.shape == (n, K, Do)
        w = np.ascontiguousarray(m[None] + noise)
    assert w.dtype == np.float32
    out = np.empty((n, K))
    wp, xp = w.ctypes.data, x32.ctypes.data
    for i in range(n):
        for k in range(K):
            out[i, k] = L.ora_ts_ctr(wp + 4 * Do * (i * K + k), xp + 4 * Do * i, Do, k, K)
    return out


def bid(kind, state, pg, gs, state16, value, ctr, gamma_raw=None, eps=None, grid=None):
    """Bidder.bid of one agent for n requests: (bid, gamma, propensity), float64 [n].

    kind, state: the agent's AG_BIDDER_* and AG_LEARNER_* (a non-learner is UNINITIALISED whatever
    `state` says); pg, gs: its prev_gamma and gamma_sigma; state16: its learner row; value, ctr
    [n]; the draw its state makes: gamma_raw [n], eps [n] float32 or grid [n][128].

      truthful                       bid = value * ctr, gamma and propensity NaN
      EmpiricalShaded                gamma = clip(gamma_raw, 0, 1), propensity NaN
      other shaders, uninitialised   gamma = gamma_raw, propensity = ora_propensity(pg, gs, gamma)
      learner in POLICY              ora_policy_bid on state16[4:] with eps
      ValueLearning in SEARCH        ora_search_gamma on state16[:4] over its grid row, propensity 1
    and bid = (value * ctr) * gamma, in that order."""
    L = lib()
    value = np.ascontiguousarray(value, np.float64).reshape(-1)
    ctr = np.ascontiguousarray(ctr, np.float64).reshape(-1)
    n = value.shape[0]
    assert ctr.shape == (n,)
    base = value * ctr
    gamma, prop = np.full(n, np.nan), np.full(n, np.nan)
    learner = kind >= VALUE_LEARNING
    if not learner:
        state = UNINITIALISED
    if learner and state == POLICY:
        st = np.ascontiguousarray(state16, np.float32).reshape(16)
        e = np.ascontiguousarray(eps, np.float32).reshape(n)
        g, p = ctypes.c_double(), ctypes.c_double()
        for i in range(n):
            L.ora_policy_bid(st.ctypes.data + 16, float(ctr[i]), float(value[i]), float(e[i]), ctypes.byref(g),
                             ctypes.byref(p))
            gamma[i], prop[i] = g.value, p.value
    elif kind == VALUE_LEARNING and state == SEARCH:
        st = np.ascontiguousarray(state16, np.float32).reshape(16)
        gr = np.ascontiguousarray(grid, np.float64).reshape(n, GRID_POINTS)
        for i in range(n):
            gamma[i] = L.ora_search_gamma(st.ctypes.data, float(ctr[i]), float(value[i]),
                                          gr.ctypes.data + 8 * GRID_POINTS * i, 1)
        prop[:] = 1.0
    elif kind != TRUTHFUL:
        gamma = np.array(gamma_raw, np.float64).reshape(n)
        if kind == EMPIRICAL_SHADED:
            gamma[gamma < 0.0] = 0.0
            gamma[gamma > 1.0] = 1.0
        else:
            prop = np.array([L.ora_propensity(float(pg), float(gs), float(g)) for g in gamma])
    else:
        return base, gamma, prop
    return base * gamma, gamma, prop


def oracle_ctr_longdouble(items, x):
    """The oracle CTR without the oracle: np.longdouble [n][K], the D products summed in order."""
    a = np.asarray(items, np.float64).astype(np.longdouble)
    x = np.asarray(x, np.float64).astype(np.longdouble)
    z = np.zeros((x.shape[0], a.shape[0]), np.longdouble)
    for d in range(a.shape[1]):
        z = z + x[:, d, None] * a[None, :, d]
    return np.longdouble(1) / (np.longdouble(1) + np.exp(-z))


def oracle_ctr_bound(items, x):
    """How far a double evaluation (any summation order, fused or not, each step correctly
    rounded) may be from oracle_ctr_longdouble, [n][K]: with S = sum |a_d x_d| the dot is off by at
    most (D + 1) 2^-53 S, which sigmoid's slope <= 1/4 carries into the CTR; exp, the add and the
    divide each round once more, every one by at most 2^-53 of a result <= 1 (4 2^-53 with room
    for exp's last-place error)."""
    a = np.abs(np.asarray(items, np.float64))
    x = np.abs(np.asarray(x, np.float64))
    D = a.shape[1]
    S = (x[:, None, :] * a[None, :, :]).sum(axis=2)
    return ((D + 1) * 2.0 ** -53 * S) / 4 + 4 * 2.0 ** -53
