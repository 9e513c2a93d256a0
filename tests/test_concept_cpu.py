"""CPU-only: the host half of TCAV (addvisor_hip/concept.py) -- the dual Newton solve on the Gram matrix against the primal
restatement of tests/concept_ref.py and against sklearn, the mean-difference CAV, the split, the score formulas, Welch's test,
the npz round trip -- and the properties of the restatement's own results that tests/test_gpu_concept.py relies on."""
import types
import warnings

import numpy as np
import pytest
import torch

import concept_ref as CR
from addvisor_hip import concept as CO

ALPHA = 0.01


def blobs(n, F, seed, shift=0.7):
    rng = np.random.default_rng(seed)
    y = np.where(np.arange(n) < n // 2, 1.0, -1.0)
    return rng.standard_normal((n, F)) + shift * y[:, None] * rng.standard_normal(F), y


def check_solution(X, y, alpha=ALPHA):
    a, b, it = CO.logistic_dual(X @ X.T, y, alpha)
    w = X.T @ a
    gw, gb = CR.primal_gradient(X, y, w, b, alpha)
    print(f"n={len(y)} F={X.shape[1]}: {it} iterations, primal gradient {gw:.3e} (max|w| {np.abs(w).max():.3e}), sum y s {gb:.3e}")
    assert gw <= 1e-12 * np.abs(w).max() and gb <= 1e-12
    return w, b


@pytest.mark.parametrize("n,F", [(17, 3136), (24, 64), (9, 5)])
def test_dual_solve_is_the_primal_minimiser(n, F):
    X, y = blobs(n, F, seed=n)
    w, b = check_solution(X, y)
    wp, bp = CR.logistic_primal(X, y, ALPHA)
    assert np.abs(w - wp).max() <= 1e-9 * np.abs(wp).max() and abs(b - bp) <= 1e-9 * max(1.0, abs(bp))


def test_dual_solve_agrees_with_sklearn():
    from sklearn.linear_model import LogisticRegression
    X, y = blobs(17, 3136, seed=3)
    w, b = check_solution(X, y)
    lr = LogisticRegression(C=1.0 / (ALPHA * len(y)), tol=1e-12, max_iter=10000).fit(X, y)
    err = np.abs(lr.coef_[0] - w).max() / np.abs(w).max()
    print(f"sklearn LogisticRegression vs the dual solve: {err:.3e} of max|w|, intercepts {lr.intercept_[0]:.9f} / {b:.9f}")
    assert err <= 1e-5 and abs(lr.intercept_[0] - b) <= 1e-5                 # lbfgs stops on its own gradient tolerance


def test_dual_solve_edge_cases():
    X, y = blobs(16, 40, seed=5, shift=6.0)                                  # linearly separable: alpha keeps the minimiser finite
    assert ((X @ (X[y > 0].mean(0) - X[y < 0].mean(0))) * y > 0).all()
    check_solution(X, y)
    Xd = np.concatenate([X, X[:4]])                                          # duplicated rows: a singular Gram matrix
    w, b = check_solution(Xd, np.concatenate([y, y[:4]]))
    wp, bp = CR.logistic_primal(Xd, np.concatenate([y, y[:4]]), ALPHA)
    assert np.abs(w - wp).max() <= 1e-9 * np.abs(wp).max()
    check_solution(X[[0, 15]], y[[0, 15]])                                   # N = 2
    for bad in (np.ones(16), -np.ones(16), np.where(np.arange(16) < 8, 1.0, 0.0)):
        with pytest.raises(ValueError):
            CO.logistic_dual(X @ X.T, bad, ALPHA)
    for alpha in (0, -1.0, float("nan"), True):
        with pytest.raises(ValueError):
            CO.logistic_dual(X @ X.T, y, alpha)
    with pytest.raises(FloatingPointError):
        CO.logistic_dual(np.full((16, 16), np.nan), y, ALPHA)
    with pytest.warns(UserWarning, match="did not converge"):
        CO.logistic_dual(X @ X.T, y, ALPHA, max_iter=1)


@pytest.mark.parametrize("C", [2, 3])
def test_fit_duals_against_the_primal_restatement(C):
    rng = np.random.default_rng(7)
    feats = [rng.standard_normal((10, 50)) + 0.8 * rng.standard_normal(50) for _ in range(C)]
    X = np.concatenate(feats)
    labels = np.repeat(np.arange(C), 10)
    train, test = CO.split_rows(len(X), 0.33, 0)
    A, b, acc = CO.fit_duals(CO.LogisticCAV(ALPHA), X @ X.T, labels, C, train, test)
    W, bref, aref = CR.fit_cav(feats, ALPHA, 0.33, 0)
    assert (A[:, test] == 0).all()
    assert np.abs(A @ X - W).max() <= 1e-9 * np.abs(W).max() and np.abs(b - bref).max() <= 1e-9 and acc == aref
    if C == 2:
        assert (A[0] == -A[1]).all() and b[0] == -b[1]                       # Captum's [-w, w]
    A0, _, acc0 = CO.fit_duals(CO.LogisticCAV(ALPHA), X @ X.T, labels, C, np.arange(len(X)), np.arange(0))
    assert 0.0 <= acc0 <= 1.0 and (A0 != 0).any()                            # an empty test set: the accuracy of the training rows


def test_mean_difference_cav():
    rng = np.random.default_rng(9)
    feats = [rng.standard_normal((7, 30)), rng.standard_normal((9, 30)) + 1.0]
    X, labels = np.concatenate(feats), np.repeat([0, 1], [7, 9])
    train, test = CO.split_rows(16, 0.25, 4)
    A, b, acc = CO.fit_duals(CO.MeanDifferenceCAV(), X @ X.T, labels, 2, train, test)
    Xt, lt = X[train], labels[train]
    w = Xt[lt == 1].mean(0) - Xt[lt == 0].mean(0)
    assert np.abs(A[1] @ X - w).max() <= 1e-13 and np.abs(A[0] @ X + w).max() <= 1e-13
    Wr, br, ar = CR.fit_cav(feats, ratio=0.25, seed=4, classifier="mean_difference")
    assert np.abs(A @ X - Wr).max() <= 1e-12 and np.abs(b - br).max() <= 1e-12 and acc == ar


def test_split_is_reproducible_and_refuses_a_missing_class():
    tr, te = CO.split_rows(24, 0.33, 0)
    tr2, te2 = CO.split_rows(24, 0.33, 0)
    assert (tr == tr2).all() and (te == te2).all() and len(te) == 7 and sorted(np.concatenate([tr, te])) == list(range(24))
    assert (te == np.random.default_rng(0).permutation(24)[:7]).all()        # the first int(ratio * N) rows of the permutation
    assert not (CO.split_rows(24, 0.33, 1)[1] == te).all()
    assert len(CO.split_rows(24, 0.0, 0)[1]) == 0
    labels = np.array([0] * 23 + [1])
    K = np.eye(24)
    seed = next(s for s in range(100) if 23 in CO.split_rows(24, 0.33, s)[1])     # the one row of class 1 lands in the test part
    with pytest.raises(ValueError, match="class 1 has no example in the training part"):
        CO.fit_duals(CO.LogisticCAV(), K, labels, 2, *CO.split_rows(24, 0.33, seed))


def test_score_formulas():
    s = np.array([[1.0, -2.0], [3.0, 0.0], [-1.0, -4.0], [2.0, 1.0]])
    sign, mean = CO.tcav_scores(s)
    assert (sign == [0.75, 0.25]).all() and (mean == [1.25, -1.25]).all()    # 0 is not > 0
    _, norm = CO.tcav_scores(s, "normalized")
    assert np.allclose(norm, [6.0 / 7.0, 1.0 / 7.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        CO.tcav_scores(s, "median")
    for mag in ("mean", "normalized"):
        a, b = CO.tcav_scores(s, mag), CR.scores_of(s, mag)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_significance_is_welchs_t_test():
    from scipy import stats
    rng = np.random.default_rng(11)
    for nx, nz, shift in ((4, 5, 0.3), (10, 10, 0.0), (3, 20, 1.0), (30, 7, 0.05), (2, 2, 0.1)):
        x, z = 0.6 + shift + 0.1 * rng.standard_normal(nx), 0.5 + 0.2 * rng.standard_normal(nz)
        t, p = CO.tcav_significance(x, z)
        ref = stats.ttest_ind(x, z, equal_var=False)
        assert abs(t - ref.statistic) <= 1e-12 * abs(ref.statistic) and abs(p - ref.pvalue) <= 1e-10 * max(ref.pvalue, 1e-300) + 1e-15, (t, p, ref)
    with pytest.raises(ValueError):
        CO.tcav_significance([0.5], [0.4, 0.6])
    assert CO.tcav_significance([0.5, 0.5], [0.4, 0.4]) == (float("inf"), 0.0)


def host_engine(tmp, **kw):
    """A HipTCAV without a device: activations are made up on the host, training is counted."""
    eng = CO.HipTCAV.__new__(CO.HipTCAV)
    att = types.SimpleNamespace(emb=types.SimpleNamespace(dev=torch.device("cpu")), precision="f32")
    eng.att, eng.layers, eng.pool, eng.ratio, eng.seed = att, [4], "none", 0.33, 0
    eng.classifier, eng.model_id, eng.save_path, eng.cavs = CO.LogisticCAV(0.01), "m", str(tmp), {}
    for k, v in kw.items():
        setattr(eng, k, v)
    eng.trained = 0
    eng._concept_activations = lambda c: {4: torch.zeros(5, 12)}

    def train(concepts, layer):
        eng.trained += 1
        return CO.CAV(torch.arange(24, dtype=torch.float32).view(2, 12) * eng.trained, [c.id for c in concepts], 0.75, np.array([-0.5, 0.5]))
    eng._train = train
    return eng


def test_npz_round_trip_and_invalidation(tmp_path):
    sets = [[CO.Concept(0, "tone", torch.zeros(5, 8)), CO.Concept(1, "random", torch.zeros(5, 8))]]
    eng = host_engine(tmp_path)
    first = eng.compute_cavs(sets)["0-1"][4]
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == ["m_0-1_layer4.npz"] and eng.trained == 1
    with np.load(tmp_path / files[0], allow_pickle=False) as z:              # no pickle inside
        assert sorted(z.files) == ["accs", "classes", "intercepts", "settings", "weights"]
    again = host_engine(tmp_path).compute_cavs(sets)["0-1"][4]
    assert torch.equal(again.weights, first.weights) and again.classes == [0, 1] and again.accs == 0.75
    assert (again.intercepts == first.intercepts).all()
    eng2 = host_engine(tmp_path)
    eng2.compute_cavs(sets)
    assert eng2.trained == 0                                                  # reloaded
    eng2.compute_cavs(sets, force_train=True)
    assert eng2.trained == 1
    for kw in (dict(seed=1), dict(ratio=0.5), dict(pool="mean"), dict(classifier=CO.LogisticCAV(0.1)), dict(classifier=CO.MeanDifferenceCAV())):
        e = host_engine(tmp_path, **kw)
        e.compute_cavs(sets)
        assert e.trained == 1, kw                                             # other settings: the stored CAV is not theirs
        host_engine(tmp_path).compute_cavs(sets, force_train=True)            # put the default's file back
    other = host_engine(tmp_path, model_id="other")
    other.compute_cavs(sets)
    assert other.trained == 1 and len(list(tmp_path.iterdir())) == 2


def test_argument_errors_without_a_device():
    with pytest.raises(TypeError):
        CO.HipTCAV(object(), [4])
    with pytest.raises(ValueError):
        CO.Concept("a", "tone", torch.zeros(2, 8))
    with pytest.raises(ValueError):
        list(CO.Concept(0, "tone", torch.zeros(8)).batches())
    with pytest.raises(ValueError):
        CO.LogisticCAV(0.0)
    eng = host_engine(".")
    c0, c1 = CO.Concept(0, "a", torch.zeros(2, 8)), CO.Concept(1, "b", torch.zeros(2, 8))
    for bad in ([], [[c0]], [[c0, c0]], [[c0, c1], [CO.Concept(0, "c", torch.zeros(2, 8)), c1]], [[c0, "x"]]):
        with pytest.raises(ValueError):
            eng._check_sets(bad)
    x = torch.zeros(2, 100)
    with pytest.raises(NotImplementedError):
        eng._check_interpret(x, 0, "gradient", "mean", {})
    for args in ((x[0], None, "gradient", "mean", {}), (x, None, "saliency", "mean", {}), (x, None, "gradient", "median", {})):
        with pytest.raises(ValueError):
            eng._check_interpret(*args)
    with pytest.raises(TypeError):
        eng._check_interpret(x, None, "gradient", "mean", {"n_steps": 4})
    eng._check_interpret(x, None, "integrated_gradients", "mean", {"n_steps": 4})
    for bad in (torch.zeros(3), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3)):      # CPU tensors never reach a kernel
        with pytest.raises(ValueError):
            CO.gram(bad)
    with pytest.raises(ValueError):
        CO.time_pool(torch.zeros(2, 3, 4))
    from captum.concept import TCAV, _layer_index
    assert _layer_index("hidden_states.4") == 4 and _layer_index(7) == 7
    for bad in ("encoder.4", "hidden_states.x", 1.5, True):
        with pytest.raises(ValueError):
            _layer_index(bad)
    with pytest.raises(TypeError):
        TCAV(object(), ["hidden_states.4"])


def test_gram_bound_has_teeth():
    """The bound of the real-valued kernel test (8 x numpy's own fp32 error, relative to sum |x y|) is missed by a float64
    reference that drops the last column: the columns set to 4.0 put 16 / sum|x y| far above it."""
    for M, _, F in CR.GRAM_REAL_SHAPES:
        X32 = CR.gram_real_inputs(M, F)
        X64 = X32.astype(np.float64)
        bound = CR.gram_bound(X32)
        dropped = CR.gram_error(X64[:, :-1] @ X64[:, :-1].T, X64, X64)
        print(f"({M},{M},{F}): numpy fp32 error {bound / 8:.3e}, bound {bound:.3e}, last column dropped {dropped:.3e}")
        assert (X32[:, 0] == 4.0).all() and (X32[:, -1] == 4.0).all()
        assert 0 < bound < 1e-5 and dropped > bound
        assert CR.gram_error(X64 @ X64.T, X64, X64) == 0.0


@pytest.mark.parametrize("pool", ["none", "mean"])
@pytest.mark.parametrize("stable", [False, True], ids=["post_ln", "pre_ln"])
def test_restatement_case(stable, pool):
    """The case of the engine parity tests: the CAVs separate, no score lies near zero (so ``sign_count`` is decided), the
    two-concept rows are negatives and the scores of the two rows mirror each other."""
    ref = CR.case_reference(stable, pool)
    assert sorted(ref) == ["0-1", "2-1"]
    for key, per in ref.items():
        for l, r in per.items():
            sc = r["scores"]
            margin = np.abs(sc).min() / np.abs(sc).max()
            print(f"{key} layer {l} pool={pool}: acc {r['accs']:.3f}, sign_count {r['sign_count']}, min|score|/max|score| {margin:.3e}")
            assert margin > 1e-3
            assert (r["weights"][0] == -r["weights"][1]).all() and (sc[:, 0] == -sc[:, 1]).all()
            assert r["sign_count"][0] + r["sign_count"][1] == 1.0
            assert 0.0 <= r["accs"] <= 1.0 and abs(round(r["accs"] * 7) - r["accs"] * 7) < 1e-9     # 7 of the 24 rows are held out
