"""CPU-only: the restatement of the perturbation curves (tests/curve_ref.py) pinned against its own definitions -- the two rank
forms, the trapezoid, a hand-computed example, the row identities, the ordering MoRF <= random <= LeRF on a linear toy model --
and the count schedules of the engine (``attribution.curve_counts``) against the restatement's."""
import numpy as np
import pytest
import torch

import curve_ref as R
from addvisor_hip import attribution as AT

trapezoid = getattr(np, "trapezoid", None) or np.trapz


def special_scores():
    rng = np.random.default_rng(3)
    inf = np.inf
    return {
        "random": rng.standard_normal((3, 37)).astype(np.float32),
        "ties": np.round(rng.standard_normal((3, 200)) * 2).clip(-4, 3).astype(np.float32),          # 8 values
        "all_equal": np.full((2, 17), 0.25, np.float32),
        "zeros_and_infs": np.array([[0.0, -0.0, inf, -inf, 1.0, -0.0, 0.0, -inf, inf, -1.0],
                                    [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 0.0]], np.float32),
        "one": np.array([[2.0]], np.float32),
    }


@pytest.mark.parametrize("name", list(special_scores()))
@pytest.mark.parametrize("descending", [True, False])
def test_rank_forms_agree(name, descending):
    s = special_scores()[name]
    a, b = R.rank_pairwise(s, descending), R.rank_argsort(s, descending)
    assert np.array_equal(a, b)
    assert all(np.array_equal(np.sort(r), np.arange(s.shape[1])) for r in a)                          # a permutation per clip


def test_rank_tie_rule():
    s = np.array([[1.0, 3.0, 1.0, 3.0, -0.0, 0.0]], np.float32)
    assert R.rank_argsort(s, True).tolist() == [[2, 0, 3, 1, 4, 5]]      # equal scores: the lower feature first, -0 == +0
    assert R.rank_argsort(s, False).tolist() == [[2, 4, 3, 5, 0, 1]]
    assert R.rank_argsort(np.full((1, 5), 7.0), True).tolist() == R.rank_argsort(np.full((1, 5), 7.0), False).tolist() == [[0, 1, 2, 3, 4]]


def test_scores_replay_against_float64():
    rng = np.random.default_rng(5)
    B, n, K = 3, 1001, 13
    a = rng.standard_normal((B, n)).astype(np.float32)
    index = rng.integers(0, K, (B, n))
    for use_abs in (False, True):
        for mean in (False, True):
            s32, s64 = R.scores32_replay(a, index, K, use_abs, mean), R.scores64(a, index, K, use_abs, mean)
            bound = n * 2.0 ** -23 * np.abs(a).sum(1, keepdims=True)     # sequential summation
            assert s32.dtype == np.float32 and (np.abs(s32 - s64) <= bound).all()
    assert np.array_equal(R.scores32_replay(a, None, n, True), np.abs(a))                             # the identity
    gap = R.scores32_replay(a[:, :4], np.array([[0, 0, 2, 2]]), 3)
    assert np.isneginf(gap[:, 1]).all() and np.isneginf(R.scores64(a[:, :4], np.array([[0, 0, 2, 2]]), 3)[:, 1]).all()


def test_auc_equals_the_trapezoid_rule():
    rng = np.random.default_rng(7)
    B, K = 4, 50
    for counts in (np.arange(0, 51, 5), np.array([0, 1, 7, 20, 49, 50]), np.array([3, 10, 11, 40])):
        S1 = len(counts)
        fk = rng.standard_normal(S1 * B)
        for prob in (False, True):
            y, auc, _ = R.fold(fk, counts, B, K, prob, False)
            f = counts / K
            assert np.allclose(auc, trapezoid(y, f, axis=1) / (f[-1] - f[0]), rtol=1e-13, atol=1e-15)
            assert np.array_equal(y, 1 / (1 + np.exp(-fk.reshape(S1, B).T)) if prob else fk.reshape(S1, B).T)


def test_hand_computed_three_features():
    x = np.array([[1, 2, 3, 4, 5, 6]], np.float32)
    attr = np.array([[1, 1, 3, 2, 0.5, 0.5]], np.float32)
    index = np.array([[0, 0, 1, 1, 2, 2]])
    forward = lambda rows: rows.sum(1)                                   # noqa: E731
    assert R.scores32_replay(attr, index, 3).tolist() == [[2.0, 5.0, 1.0]]
    curve, frac, auc, aopc, rank = R.perturbation_curve(forward, x, attr, "deletion", "morf", index, 3, steps=3, prob=False)
    assert rank.tolist() == [[1, 0, 2]]
    assert curve.tolist() == [[21.0, 14.0, 11.0, 0.0]] and np.allclose(frac, [0, 1 / 3, 2 / 3, 1])
    assert np.isclose(auc[0], 35.5 / 3) and np.isclose(aopc[0], 38.0 / 3)
    curve, _, auc, aopc, rank = R.perturbation_curve(forward, x, attr, "insertion", "morf", index, 3, steps=3, prob=False)
    assert curve.tolist() == [[0.0, 7.0, 10.0, 21.0]]                    # the reference step is the last one
    assert np.isclose(auc[0], (3.5 + 8.5 + 15.5) / 3) and np.isclose(aopc[0], (21 + 14 + 11) / 3)
    curve, _, _, _, rank = R.perturbation_curve(forward, x, attr, "deletion", "lerf", index, 3, steps=3, prob=False)
    assert rank.tolist() == [[1, 2, 0]] and curve.tolist() == [[21.0, 10.0, 7.0, 0.0]]
    mean = R.scores32_replay(attr, np.array([[0, 1, 1, 1, 2, 2]]), 3, mean=True)
    assert mean.tolist() == [[1.0, 2.0, 0.5]]


def test_row_identities():
    rng = np.random.default_rng(11)
    B, n, K = 3, 103, 9
    x, base = rng.standard_normal((B, n)).astype(np.float32), rng.standard_normal((B, n)).astype(np.float32)
    index = rng.integers(0, K, (B, n))
    score = rng.standard_normal((B, K)).astype(np.float32)               # tie-free
    morf, lerf = R.rank_argsort(score, True), R.rank_argsort(score, False)
    assert np.array_equal(morf + lerf, np.full((B, K), K - 1))
    counts = np.array([0, 2, 5, K], np.int32)
    dele, ins = R.rows(x, base, index, morf, counts, 0), R.rows(x, base, index, morf, counts, 1)
    assert np.array_equal(dele[:B], x) and np.array_equal(dele[-B:], base)
    assert np.array_equal(ins[:B], base) and np.array_equal(ins[-B:], x)
    # deletion in MoRF order at c == insertion in LeRF order at K - c: the same features are at the baseline
    back = R.rows(x, base, index, lerf, (K - counts[::-1]).astype(np.int32), 1)
    for j in range(len(counts)):
        assert np.array_equal(dele[j * B:(j + 1) * B], back[(len(counts) - 1 - j) * B:(len(counts) - j) * B])
    pad = R.rows(x, base[:1], index[:1], morf, counts, 0, n_rows=5, row0=len(counts) * B - 2)
    assert np.array_equal(pad[:2], R.rows(x, base[:1], index[:1], morf, counts, 0)[-2:])
    assert np.array_equal(pad[2:], x[[(len(counts) * B + i) % B for i in range(3)]])
    bad = index.copy()
    bad[1, 5], bad[2, 7] = K, -1
    out = R.rows(x, base, bad, morf, counts, 0)
    want = np.zeros_like(out, bool)
    want[1::B, 5], want[2::B, 7] = True, True
    assert np.array_equal(np.isnan(out), want)


def test_linear_model_orders_morf_random_lerf():
    """``F(x) = w . x`` with ``attr = w * x`` pooled over segments is exact: removing the c largest contributions leaves the
    smallest sum any c features can leave, so the deletion curve in MoRF order lies below every other order's, LeRF's above.
    B = 4, K = 16 segments of 25 samples; segment sums of N(0, 1) products differ by O(1), far from fp32 rounding."""
    rng = np.random.default_rng(13)
    B, n, K = 4, 400, 16
    w = (0.1 * rng.standard_normal(n)).astype(np.float32)                # logits of a few units: the sigmoid does not saturate
    x = rng.standard_normal((B, n)).astype(np.float32)
    index = (np.arange(n) // 25)[None]
    forward = lambda rows: rows.astype(np.float64) @ w.astype(np.float64)    # noqa: E731
    attr = w[None] * x
    for prob in (False, True):
        auc = {o: R.perturbation_curve(forward, x, attr, "deletion", o, index, K, steps=K, prob=prob)[2] for o in ("morf", "lerf")}
        assert (auc["morf"] < auc["lerf"]).all()
        for seed in (0, 1, 2, 3):
            rank = AT.shapley_permutations(seed, B, K)
            rnd = R.perturbation_curve(forward, x, attr, "deletion", "random", index, K, steps=K, prob=prob, rank=rank)[2]
            margin = 1e-3 * (auc["lerf"] - auc["morf"])
            print(f"prob={prob} seed={seed}: morf {auc['morf']}, random {rnd}, lerf {auc['lerf']}")
            assert (auc["morf"] + margin < rnd).all() and (rnd + margin < auc["lerf"]).all()
        # insertion mirrors it: the most relevant features first raise the output fastest
        ins = {o: R.perturbation_curve(forward, x, attr, "insertion", o, index, K, steps=K, prob=prob)[2] for o in ("morf", "lerf")}
        assert (ins["morf"] > ins["lerf"]).all()


def test_count_schedules():
    for K in (1, 2, 7, 10, 20, 21, 40, 16000):
        for steps in (None, 1, min(K, 3), K):
            c = AT.curve_counts(steps, K)
            S = min(K, 20) if steps is None else steps
            assert c.dtype == np.int32 and np.array_equal(c, R.counts_from_steps(steps, K))
            assert c[0] == 0 and c[-1] == K and len(c) == S + 1 and (np.diff(c) > 0).all()
            assert c.tolist() == [(j * K + S // 2) // S for j in range(S + 1)]
    assert AT.curve_counts([0.0, 0.25, 0.5, 1.0], 10).tolist() == [0, 3, 5, 10]        # floor(2.5 + 0.5) = 3
    assert AT.curve_counts(torch.tensor([0.0, 0.1, 1.0]), 16).tolist() == [0, 2, 16]
    assert AT.curve_counts(np.linspace(0, 1, 5), 8).tolist() == R.counts_from_steps(np.linspace(0, 1, 5), 8).tolist() == [0, 2, 4, 6, 8]


@pytest.mark.parametrize("steps,K", [(0, 5), (6, 5), (-1, 5), (True, 5), (2.5, 5), ("3", 5), ([0.0, 1.0, 0.5], 5), ([0.1, 1.0], 5),
                                     ([0.0, 0.9], 5), ([0.0, 0.5, 0.5, 1.0], 5), ([0.0, 0.01, 1.0], 5), ([0.0, 0.5, 0.55, 1.0], 4),
                                     ([1.0], 5), ([[0.0, 1.0]], 5), ([0.0, float("nan"), 1.0], 5)])
def test_count_schedule_errors(steps, K):
    with pytest.raises(ValueError):
        AT.curve_counts(steps, K)
