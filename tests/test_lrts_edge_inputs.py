"""The inputs of tests/test_gpu_lrts_edges.py do what their GPU tests need, shown on the oracle alone
(no GPU): a device test must not pass because an input stopped early or never saturated."""
import numpy as np
import pytest

import lrts_edge_cases as E


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


@pytest.mark.parametrize("name", sorted(E.BUILDERS))
def test_every_input_trains_to_finite_values(name):
    m, pm, q, ep, L = E.oracle_result(name)
    c = E.case(name)
    assert 0 < ep <= E.MAX_EPOCHS and len(L) == ep
    assert np.isfinite(m).all() and np.isfinite(q).all() and np.isfinite(L).all()
    assert np.array_equal(pm, m) and not np.array_equal(m, c["m"])
    assert (c["X"][:, -1] == 1).all() and c["A"].max() < c["m"].shape[0]


def test_groups_cover_every_small_input_once():
    grouped = [n for names in E.GROUPS.values() for n in names]
    assert sorted(grouped) == sorted(set(E.BUILDERS) - set(E.BIG))
    for (K, Do), names in E.GROUPS.items():
        for n in names:
            assert E.case(n)["m"].shape == (K, Do)
        assert K * Do <= 12 or (K, Do) == (12, 5)  # the one larger model: items without samples


@pytest.mark.parametrize("name", E.CAP)
def test_cap_inputs_run_every_epoch(name):
    """All 16384 epochs: the last Adam-table entry, the last trace column, a loss history wrapped
    163 times; no early stop although the check is armed from epoch 1025 on."""
    ep, L = E.oracle_result(name)[3:]
    assert ep == E.MAX_EPOCHS
    assert (np.abs(L[1025 - 99:-99].astype(np.float64) - L[1025:].astype(np.float64)) >= 1e-6).all()


# (halvings, refusals at the lr floor) of every input: 2e-3 halves 17 times before
# `lr - lr / 2 > 1e-8` refuses. Listed here: a cap input whose loss falls all the way, never stalling for
# 11 epochs. The early-stopping inputs all reach the floor, and so does the cap input x64_cap.
NEVER_HALVES = ("cap_k1", "cap_k2", "all_y0", "all_y1", "n2_two_items", "n3")


def test_scheduler_replay_states_which_inputs_hit_the_lr_floor():
    """ReduceLROnPlateau replayed over the oracle's trace of EVERY input: each either never halves
    (NEVER_HALVES above) or halves 17 times and is then refused at the floor at least once."""
    for n in E.BUILDERS:
        got = E.scheduler_replay(E.oracle_result(n)[4])
        if n in NEVER_HALVES:
            assert got == (0, 0) and n in E.CAP, (n, got)
        else:
            assert got[0] == 17 and got[1] >= 1, (n, got)
    assert E.scheduler_replay(E.oracle_result("saturated")[4])[1] >= 40   # most of its epochs at the floor
    assert E.scheduler_replay(E.oracle_result("x64_cap")[4])[1] >= 1000   # a capped fit at the floor


def test_every_input_is_capped_or_stops_early_as_listed():
    for n in E.BUILDERS:
        ep = E.oracle_result(n)[3]
        assert (ep == E.MAX_EPOCHS) == (n in E.CAP), (n, ep)
        assert ep > 1026 or n in ("saturated", "n2_same_item"), (n, ep)  # (those two stop at the first chance)


def test_saturated_input_has_every_class_at_epoch_0():
    c = E.case("saturated")
    z, p = E.epoch0_classes(c)
    y = c["y"]
    assert z.dtype == np.float32 and p.dtype == np.float32
    assert ((p == 0.0) & y).any()            # log(0) = -inf: the -100 clamp, y = 1 side
    assert ((p == 1.0) & ~y).any()           # log1p(-1) = -inf: the clamp, y = 0 side
    for bound in (512.0, 745.0):             # exp's special path; its underflow and overflow
        assert (z >= bound).any() and (z <= -bound).any()
        assert ((z >= bound) & y).any() and ((z >= bound) & ~y).any()
        assert ((z <= -bound) & y).any() and ((z <= -bound) & ~y).any()
    assert (z == 0.0).any()                  # exp(-0.0) and exp(+0.0): the tiny-argument path
    assert ((z == 0.0) & y).any() and ((z == 0.0) & ~y).any()
    # the clamp decides the first loss: every clamped sample adds exactly 100
    clamped = int(((p == 0.0) & y).sum() + ((p == 1.0) & ~y).sum())
    assert clamped >= 50 and E.oracle_result("saturated")[4][0] >= 100.0 * clamped


def test_unsampled_rows_keep_bias_and_q():
    """Items 5-11 have no sample: their bias column (no prior) and every q stay bit for bit, the
    other columns move (the prior's gradient alone); the sampled rows' q grows."""
    c = E.case("unsampled_items")
    m, _, q, _, _ = E.oracle_result("unsampled_items")
    assert c["A"].max() == 4 and len(set(c["y"])) == 2
    assert np.array_equal(m[5:, -1], c["m"][5:, -1]) and np.array_equal(q[5:], c["q"][5:])
    assert (m[5:, :-1] != c["m"][5:, :-1]).all()
    assert (q[:5] > c["q"][:5]).all()
    for name in ("all_y0", "all_y1"):
        assert len(set(E.case(name)["y"])) == 1 and E.case(name)["A"].max() == 4


def test_tiny_and_q_inputs_are_what_they_say():
    assert len(E.case("n2_same_item")["y"]) == 2 and len(set(E.case("n2_same_item")["A"])) == 1
    assert sorted(E.case("n2_same_item")["y"]) == [False, True]
    assert len(set(E.case("n2_two_items")["A"])) == 2 and E.case("n2_two_items")["y"].all()
    assert len(E.case("n3")["y"]) == 3
    assert (E.case("q_zero")["q"] == 0).all() and (E.case("q_1e6")["q"] == 1e6).all()
    # q = 1e6 pins the non-bias columns to prev_m far harder than q = 0
    for name, far in (("q_zero", True), ("q_1e6", False)):
        c, m = E.case(name), E.oracle_result(name)[0]
        assert (np.abs(m[:, :-1] - c["pm"][:, :-1]).max() > 1e-2) == far


@pytest.mark.parametrize("name", E.MAGNITUDE)
def test_magnitude_inputs_stay_inside_the_exact_sum_range(name):
    """The range include/auctiongym.h states for ag_lrts_update, for ANY placement of the samples
    on lanes (one lane holding all of an item's samples is the worst): per item and column
    sum |x| <= 2^22 and sum x^2 <= 2^24, every |x| < 2^23 -- and the input is large all the same."""
    c = E.case(name)
    X = c["X"].astype(np.float64)
    assert np.abs(X).max() < 2.0 ** 23 and np.abs(X).max() >= 64.0
    for k in range(c["m"].shape[0]):
        rows = X[c["A"] == k]
        assert (np.abs(rows).sum(0) <= E.RANGE_ABS).all()
        assert ((rows.astype(np.float32) ** 2).astype(np.float64).sum(0) <= E.RANGE_SQ).all()


def test_big_inputs_have_the_sizes_their_splits_need():
    assert len(E.case("big_k12")["y"]) == 4396           # 4096 cached + 300 streamed; 2 x 2048 + 300
    assert len(E.case("rp_k12")["y"]) == 2 * 2048 + 100 and len(E.case("rp_k12_b")["y"]) == 2048 + 100
    assert len(E.case("big_k2")["y"]) == 34900           # 18 workgroups of 2048: a second tree level
    assert -(-34900 // 2048) == 18 > 16
