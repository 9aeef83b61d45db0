"""Inputs that drive the LR-TS update (csrc/ag_lrts.hip, oracle/ag_oracle.c ora_lrts_update) into
the branches ordinary data never reaches: the epoch cap, a saturated float32 sigmoid, the BCE clamp,
exp outside its main path, items with no sample, one-sided labels, two and three samples, q = 0 and
1e6, and large features inside the exact sums' range.

Plain data builders, no GPU: tests/test_lrts_edge_inputs.py proves on the oracle alone that each
input reaches its branch, tests/test_gpu_lrts_edges.py runs them through both device trainers.
A case is a dict: X [n][Do] float32 (last column 1), A [n] items, y [n] labels, m, pm, q [K][Do].
oracle_result(name) is computed once per process and must not be modified.
"""
import functools

import numpy as np

MAX_EPOCHS = 16384
# include/auctiongym.h, ag_lrts_update: per item and column, the samples one lane holds keep
# sum |x| <= 2^22 and sum x^2 <= 2^24 (every |x| < 2^23). A lane can hold any subset of an
# agent's samples, so a magnitude input keeps the sums over ALL its samples inside.
RANGE_ABS, RANGE_SQ = 2.0 ** 22, 2.0 ** 24


def _case(X, A, y, m, pm=None, q=None):
    m = np.asarray(m, np.float32)
    return dict(X=np.ascontiguousarray(X, np.float32), A=np.asarray(A, np.int32), y=np.asarray(y) != 0, m=m,
                pm=m.copy() if pm is None else np.asarray(pm, np.float32),
                q=np.ones_like(m) if q is None else np.asarray(q, np.float32))


def features(g, n, Do, scale=1.0):
    return np.concatenate([scale * g.normal(0, 1, (n, Do - 1)), np.ones((n, 1))], axis=1).astype(np.float32)


def ordinary(g, n, K, Do, items=None, p=0.35):
    """The benign recipe of the rest of the suite: N(0,1) features, |m| ~ 1, q in [1, 2]."""
    m = g.normal(0, 1, (K, Do)).astype(np.float32)
    q = (1 + g.random((K, Do))).astype(np.float32)
    A = g.integers(0, K if items is None else items, n)
    return _case(features(g, n, Do), A, g.random(n) < p, m, (m + 0.5).astype(np.float32), q)


# ---- shape (1, 1) and (2, 2): the small cap inputs (both trainers) and the 18-workgroup agent
def cap_k1():
    """64 samples, all y = 1, bias -20: the loss falls by more than 1e-6 per 100 epochs to the end."""
    return _case(np.ones((64, 1)), np.zeros(64), np.ones(64), [[-20.0]])


def cap_k2():
    g = np.random.default_rng(11)
    return _case(features(g, 200, 2), g.integers(0, 2, 200), np.ones(200), [[0.0, -20.0], [0.0, -20.0]])


def big_k2():
    """34 900 samples: 18 workgroups of the per-epoch form (two levels of its combining tree)."""
    return ordinary(np.random.default_rng(12), 34900, 2, 2)


# ---- shape (12, 5): items without samples, one-sided labels, the streamed chunk
def _rows_0_to_4(labels):
    c = ordinary(np.random.default_rng(21), 300, 12, 5, items=5)
    if labels is not None:
        c["y"] = np.full(300, bool(labels))
    return c


def all_y0():
    return _rows_0_to_4(0)


def all_y1():
    return _rows_0_to_4(1)


def unsampled_items():
    """Mixed labels on items 0-4 only: rows 5-11 see the prior's gradient alone."""
    return _rows_0_to_4(None)


def big_k12():
    """4396 samples: 300 past the 4096 one workgroup keeps in registers."""
    return ordinary(np.random.default_rng(22), 4396, 12, 5)


def rp_k12():
    """2 * 2048 + 100 samples: three workgroups of the per-epoch form."""
    c = big_k12()
    return _case(c["X"][:4196], c["A"][:4196], c["y"][:4196], c["m"], c["pm"], c["q"])


def rp_k12_b():
    """2148 samples: two workgroups, beside rp_k12 (each agent its own tree rows)."""
    return ordinary(np.random.default_rng(23), 2148, 12, 5)


# ---- shape (6, 2): saturation, q, sample-count and magnitude edges
SAT_BIAS = (-120.0, 40.0, -600.0, 800.0, -800.0, 0.0)


def saturated():
    """400 samples with p(y) = 0.5; the rows are zero but for biases that put the logit where the
    float32 sigmoid is exactly 0 or 1, where |z| >= 512 and >= 745 (exp's special and under/overflow
    paths), and -- the all-zero row -- at z = 0."""
    g = np.random.default_rng(31)
    m = np.zeros((6, 2), np.float32)
    m[:, 1] = SAT_BIAS
    A = np.arange(400) % 6
    return _case(features(g, 400, 2), A, g.random(400) < 0.5, m)


def _k6(seed, n):
    return ordinary(np.random.default_rng(seed), n, 6, 2)


def q_zero():
    c = _k6(32, 300)
    c["q"][:] = 0.0
    return c


def q_1e6():
    c = _k6(33, 300)
    c["q"][:] = 1e6
    return c


def n2_same_item():
    c = _k6(34, 2)
    c["A"][:] = 3
    c["y"] = np.array([False, True])
    return c


def n2_two_items():
    c = _k6(35, 2)
    c["A"][:] = (1, 4)
    c["y"] = np.array([True, True])
    return c


def n3():
    return _k6(36, 3)


def x1024_few():
    """Eight of 300 samples with features 1024 times larger."""
    c = _k6(37, 300)
    c["X"][:8, :-1] *= 1024.0
    return c


def x64_all():
    """Every feature 64 times larger."""
    c = _k6(38, 200)
    c["X"][:, :-1] *= 64.0
    return c


def x64_cap():
    """Every feature 64 times larger on a K = 2, OE + 1 = 6 model: never stops early although the
    scheduler is at its lr floor for most of the fit."""
    c = ordinary(np.random.default_rng(40), 120, 2, 6)
    c["X"][:, :-1] *= 64.0
    return c


def tree_100():
    """100 samples: 7 workgroups of 16 (the last one short)."""
    return _k6(41, 100)


def tree_400():
    """400 samples: 25 workgroups of 16, two levels of the trainer's combining tree."""
    return _k6(42, 400)


BUILDERS = {f.__name__: f for f in (cap_k1, cap_k2, big_k2, all_y0, all_y1, unsampled_items, big_k12, rp_k12, rp_k12_b,
                                    saturated,
                                    q_zero, q_1e6, n2_same_item, n2_two_items, n3, x1024_few, x64_all, x64_cap,
                                    tree_100, tree_400)}
CAP = ("cap_k1", "cap_k2", "all_y0", "all_y1", "n2_two_items", "n3", "x64_cap")   # must run all 16384 epochs
MAGNITUDE = ("x1024_few", "x64_all", "x64_cap")
BIG = ("big_k2", "big_k12", "rp_k12", "rp_k12_b", "tree_100", "tree_400")  # each on an engine of its own
# one engine per shape; several cases per launch
GROUPS = {(1, 1): ("cap_k1",), (2, 2): ("cap_k2",), (2, 6): ("x64_cap",), (12, 5): ("all_y0", "all_y1", "unsampled_items"),
          (6, 2): ("saturated", "q_zero", "q_1e6", "n2_same_item", "n2_two_items", "n3", "x1024_few", "x64_all")}


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """oracle.lrts_update of the case: (m, prev_m, q, epochs, losses float32 [epochs])."""
    import oracle
    c = case(name)
    m, pm, q, ep, L = oracle.lrts_update(c["X"], c["A"], c["y"], c["m"], c["pm"], c["q"])
    return m, pm, q, ep, L.astype(np.float32)


def sample(name):
    c = case(name)
    return c["X"], c["A"], c["y"]


def scheduler_replay(losses):
    """ReduceLROnPlateau as ora_lrts_update states it, over a loss trace: (halvings, times the
    `lr - lr / 2 > 1e-8` guard refused one: the lr floor)."""
    lr, best, bad, halved, floored = 2e-3, np.inf, 0, 0, 0
    for loss in np.asarray(losses, np.float64):
        if loss < best * (1.0 - 1e-4):
            best, bad = loss, 0
        else:
            bad += 1
        if bad > 10:
            if lr - lr * 0.5 > 1e-8:
                lr, halved = lr * 0.5, halved + 1
            else:
                floored += 1
            bad = 0
    return halved, floored


def epoch0_classes(c):
    """Each sample's logit and float32 sigmoid at the starting m, as lrts_loss_grad states them."""
    X, w = c["X"], c["m"][c["A"]]
    z = X[:, 0] * w[:, 0]
    for d in range(1, X.shape[1]):
        z = (z + X[:, d] * w[:, d]).astype(np.float32)
    with np.errstate(over="ignore"):
        p = (np.float32(1) / (np.float32(1) + np.exp(-z.astype(np.float64)).astype(np.float32))).astype(np.float32)
    return z, p
