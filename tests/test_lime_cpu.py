"""CPU-only: Lime and FeaturePermutation: the host models of captum._utils.models.linear_model against sklearn and their
optimality conditions, the similarity kernel against torch's formula, the host draws, the Captum names and signatures, argument
checking in the engine and the captum.attr front end before any GPU work, the error contract of the new entry points, and their
resource usage."""
import ctypes as C
import inspect
import time

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

import lime_ref as R
from addvisor_hip import _lib, attribution as AT, linear_model as LM
from test_build_resources import resources


def problem(S, K, seed, sparse=0.3):
    rng = np.random.default_rng(seed)
    z = (rng.random((S, K)) < 0.5).astype(np.float64)
    c = rng.normal(size=K) * (rng.random(K) < sparse)
    y = 0.3 + 0.05 * z @ c + 0.01 * rng.normal(size=S)
    w = np.exp(-rng.random(S))
    return z, y, w


def fit(model, z, y, w):
    """Captum's protocol: fit on a DataLoader of float32 tensors, read representation() and bias()."""
    data = TensorDataset(torch.from_numpy(z.astype(np.float32)), torch.from_numpy(y.astype(np.float32)),
                         torch.from_numpy(w.astype(np.float32)))
    model.fit(DataLoader(data, batch_size=len(y)))
    rep = model.representation()
    assert rep.dtype == torch.float32 and rep.shape == (1, z.shape[1])
    assert model.bias().shape == (1,)
    return model.coef_, model.intercept_


@pytest.mark.parametrize("S,K,alpha", [(50, 12, 0.01), (50, 40, 0.01), (200, 40, 0.002), (30, 8, 0.05)])
def test_lasso_against_sklearn(S, K, alpha):
    sk = pytest.importorskip("sklearn.linear_model")
    z, y, w = problem(S, K, S + K)
    coef, icpt, _, _ = LM.lasso_fit(z, y, w, alpha)
    m = sk.Lasso(alpha=alpha, tol=1e-12, max_iter=10 ** 6).fit(z, y, sample_weight=w)
    assert np.abs(coef - m.coef_).max() <= 1e-8 and abs(icpt - m.intercept_) <= 1e-8, (np.abs(coef - m.coef_).max(), icpt - m.intercept_)
    # Captum's own call: float32 data, sklearn's default tol = 1e-4
    z32, y32, w32 = z.astype(np.float32), y.astype(np.float32), w.astype(np.float32)
    m32 = sk.Lasso(alpha=alpha).fit(z32, y32, sample_weight=w32)
    ours = fit(LM.SkLearnLasso(alpha=alpha), z, y, w)[0]
    assert np.abs(ours - m32.coef_).max() <= 1e-3 * max(np.abs(ours).max(), 1e-12)


@pytest.mark.parametrize("S,K,alpha", [(50, 12, 0.01), (50, 40, 0.01), (40, 300, 0.005), (200, 6, 1e-4), (50, 4, 10.0)])
def test_lasso_kkt(S, K, alpha):
    z, y, w = problem(S, K, 7 * S + K)
    coef, icpt = fit(LM.SkLearnLasso(alpha=alpha), z, y, w)
    # the fit saw float32 data: check the conditions on the same numbers
    z32, y32, w32 = (a.astype(np.float32).astype(np.float64) for a in (z, y, w))
    g, r0 = R.lasso_gradient(z32, y32, w32, coef, icpt)
    on = coef != 0
    assert np.all(np.abs(g[on] + alpha * np.sign(coef[on])) <= 1e-9), np.abs(g[on] + alpha * np.sign(coef[on])).max()
    assert np.all(np.abs(g[~on]) <= alpha * (1 + 1e-9)), np.abs(g[~on]).max()
    assert abs(r0) <= 1e-12
    if alpha == 10.0:
        assert not on.any() and np.isclose(icpt, np.average(y32, weights=w32))      # alpha above the largest correlation


def test_lasso_is_fast_at_thousands_of_features():
    z, y, w = problem(50, 4000, 11, sparse=0.02)
    t0 = time.perf_counter()
    coef, icpt = fit(LM.SkLearnLasso(alpha=0.01), z, y, w)
    dt = time.perf_counter() - t0
    print(f"Lasso S = 50, K = 4000: {dt:.3f} s, {np.count_nonzero(coef)} non-zero")
    assert dt < 10.0
    assert R.kkt_violation(*(a.astype(np.float32).astype(np.float64) for a in (z, y, w)), 0.01, coef, icpt) <= 1e-7


def test_lasso_warns_when_max_iter_is_reached():
    z, y, w = problem(50, 40, 3)
    with pytest.warns(UserWarning):
        LM.lasso_fit(z, y, w, 1e-4, max_iter=1)


def test_ridge_and_linear_regression():
    for S, K in ((50, 12), (20, 60)):
        z, y, w = problem(S, K, S * K)
        coef, icpt = fit(LM.SkLearnRidge(alpha=0.5), z, y, w)
        z32, y32, w32 = (a.astype(np.float32).astype(np.float64) for a in (z, y, w))
        zc, yc, _ = R.centred(z32, y32, w32)
        want = np.linalg.solve(zc.T @ (w32[:, None] * zc) + 0.5 * np.eye(K), zc.T @ (w32 * yc))     # the normal equations
        assert np.allclose(coef, want, rtol=1e-9, atol=1e-11)
        zm, ym = np.average(z32, axis=0, weights=w32), np.average(y32, weights=w32)
        assert np.isclose(icpt, ym - zm @ want, rtol=1e-9, atol=1e-11)
        try:
            from sklearn.linear_model import Ridge
        except ImportError:
            pass
        else:
            m = Ridge(alpha=0.5, solver="cholesky").fit(z32, y32, sample_weight=w32)
            assert np.allclose(coef, m.coef_, rtol=1e-8, atol=1e-10) and np.isclose(icpt, m.intercept_, rtol=1e-8, atol=1e-10)
    # SkLearnLinearRegression is KernelShap's host fit, bit for bit, on KernelShap's own coalitions and weights
    z = AT.kernel_shap_draws(5, [7], 40)[0]
    y = np.random.default_rng(1).normal(size=40).astype(np.float32)
    coef, icpt = fit(LM.SkLearnLinearRegression(), z.astype(np.float64), y.astype(np.float64), AT.kernel_shap_weights(z))
    kc, ki = AT.kernel_shap_fit(z, y.astype(np.float64))
    assert np.array_equal(coef, kc) and icpt == ki


def test_similarity_against_torch():
    g = torch.Generator().manual_seed(3)
    L = 1001
    x = torch.randn(L, generator=g)
    base = 0.1 * torch.randn(L, generator=g)
    m = (torch.rand(L, generator=g) < 0.5).float()
    rows = {"presence": base * (1 - m) + x * m, "zero": torch.zeros(L), "x": x.clone(), "base": base}
    for mode in ("cosine", "euclidean"):
        for width in (1.0, 0.3, 40.0):
            f = AT.ExpKernelSimilarity(mode, width)
            for name, v in rows.items():
                ref = R.similarity(x, v, mode, width)
                # torch's own formula in float64
                xd, vd = x.double(), v.double()
                d = 1 - torch.nn.CosineSimilarity(dim=0)(xd, vd) if mode == "cosine" else torch.norm(xd - vd)
                want = float(torch.exp(-d ** 2 / (2 * width ** 2)))
                assert abs(ref - want) <= 1e-12 * max(want, 1e-300), (mode, width, name)
                assert abs(f(x[None], v[None], None) - ref) <= 1e-5 * ref + 1e-30, (mode, width, name)
    assert R.similarity(x, torch.zeros(L), "cosine", 1.0) == pytest.approx(np.exp(-0.5), rel=1e-15)       # cos = 0 at a zero row
    from captum.attr._core.lime import get_exp_kernel_similarity_function
    f = get_exp_kernel_similarity_function()
    assert isinstance(f, AT.ExpKernelSimilarity) and (f.distance_mode, f.kernel_width) == ("cosine", 1.0)


def test_draws():
    Ks, S = [3, 40, 1], 5000
    z = AT.lime_draws(9, Ks, S)
    rng = np.random.Generator(np.random.PCG64(9))
    for K, zb in zip(Ks, z):
        assert zb.dtype == np.uint8 and zb.shape == (S, K)
        assert np.array_equal(zb, (rng.random((S, K)) < 0.5).astype(np.uint8))          # clips in order, one stream
        assert abs(zb.mean() - 0.5) < 5 * 0.5 / np.sqrt(zb.size)
    assert all(np.array_equal(a, b) for a, b in zip(z, AT.lime_draws(9, Ks, S)))
    assert not np.array_equal(AT.lime_draws(10, Ks, S)[1], z[1])
    for B in (2, 3, 5):
        p = AT.feature_permutation_draws(4, 3000, B)
        assert p.dtype == np.int32 and p.shape == (3000, B)
        assert np.array_equal(np.sort(p, axis=1), np.tile(np.arange(B), (3000, 1)))    # permutations
        assert not (p == np.arange(B)).all(1).any()                                    # never the identity
        assert np.array_equal(p, AT.feature_permutation_draws(4, 3000, B))
    p = AT.feature_permutation_draws(4, 4000, 2)
    assert (p == [1, 0]).all()                                                          # B = 2: the swap, always
    p = AT.feature_permutation_draws(5, 6000, 3)
    counts = np.unique(p, axis=0, return_counts=True)[1]
    assert len(counts) == 5 and np.all(np.abs(counts - 1200) < 5 * np.sqrt(1200))       # uniform over the 5 non-identities
    with pytest.raises(ValueError):
        AT.feature_permutation_draws(1, 3, 1)
    torch.manual_seed(0)                                                                # torch.manual_seed fixes the seed
    s1 = AT._check_seed(None)
    torch.manual_seed(0)
    assert AT._check_seed(None) == s1


def test_feature_indices_for_lime():
    B, L = 2, 8
    m = torch.tensor([[-3, -3, 5, 5, 0, 0, 5, -3], [2, 2, 2, 2, 2, 2, 2, 2]])
    index, Ks = AT.per_clip_feature_indices(m, B, L)
    assert Ks == [3, 1] and index[0].tolist() == [0, 0, 2, 2, 1, 1, 2, 0] and index[1].tolist() == [0] * 8
    index, Ks = AT.per_clip_feature_indices(None, B, L)
    assert Ks == [L, L] and index.shape == (1, L)
    assert AT.kernel_shap_feature_indices(m.abs() + torch.tensor([[0] * 8, [0] * 7 + [1]]), B, L)[1] == [3, 2]   # unchanged


def test_rows_restatement():
    x = np.arange(12, dtype=np.float32).reshape(3, 4)
    perm = np.array([[1, 2, 0], [2, 0, 1]], np.int32)
    rows = R.permuted_rows(x, np.array([0, 1, 1, 0]), perm)
    assert rows[0].tolist() == [4, 1, 2, 7] and rows[4].tolist() == [4, 1, 2, 7] and rows[5].tolist() == [8, 5, 6, 11]


def test_engine_validates_before_gpu_work():
    """Argument errors surface before the engine touches the device (the engine object is never used)."""
    att = AT.HipAttribution.__new__(AT.HipAttribution)
    x = torch.zeros(2, 100)
    seg = (torch.arange(100) // 10)[None]

    def gen(inp, **kw):
        yield torch.ones(1, 10)
    calls = [lambda: att.feature_permutation(x[:1], feature_mask=seg), lambda: att.feature_permutation(x[0], feature_mask=seg),
             lambda: att.feature_permutation(x, feature_mask=seg.expand(2, 100)),                 # one mask for every clip
             lambda: att.feature_permutation(x, feature_mask=seg.float()), lambda: att.feature_permutation(x, feature_mask=seg[:, :99]),
             lambda: att.feature_permutation(x, feature_mask=seg, internal_batch_size=0),
             lambda: att.lime(x, feature_mask=seg, return_input_shape=False),                     # B > 1
             lambda: att.lime(x, feature_mask=seg, similarity_func=3), lambda: att.lime(x, feature_mask=seg, perturb_func=gen),
             lambda: att.lime(x, feature_mask=seg, perturb_func="bernoulli"), lambda: att.lime(x, feature_mask=seg, interpretable_model=object()),
             lambda: att.lime(x, feature_mask=seg.float()), lambda: att.lime(x, baselines=torch.zeros(3, 100)),
             lambda: att.lime(x, feature_mask=seg, internal_batch_size=0), lambda: att.lime(x, feature_mask=seg, seed=-1)]
    for bad in (0, -1, 2.5, True, None):
        calls.append(lambda bad=bad: att.lime(x, feature_mask=seg, n_samples=bad))
    for mode, width in (("manhattan", 1.0), ("cosine", 0.0), ("cosine", -1.0), ("euclidean", float("inf")), ("cosine", float("nan")),
                        ("cosine", 1e39), ("cosine", True)):
        calls.append(lambda mode=mode, width=width: AT.ExpKernelSimilarity(mode, width))
        bad = AT.ExpKernelSimilarity()
        bad.distance_mode, bad.kernel_width = mode, width
        calls.append(lambda bad=bad: att.lime(x, feature_mask=seg, similarity_func=bad))
    for call in calls:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(AttributeError):                                  # valid arguments reach the (absent) device
        att.lime(x, feature_mask=seg - 5, n_samples=1)


class _NoEngine:
    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.attr import FeaturePermutation, Lime, NoiseTunnel
    from captum.attr._core.lime import get_exp_kernel_similarity_function
    x = torch.zeros(2, 100)
    seg = (torch.arange(100) // 10)[None]

    def gen(inp, **kw):
        yield torch.ones(1, 10)
    lime, fp = Lime(_NoEngine()), FeaturePermutation(_NoEngine())
    calls = [lambda: FeaturePermutation(_NoEngine(), perm_func=lambda x, m: x),
             lambda: fp.attribute(x[:1], feature_mask=seg), lambda: fp.attribute(x, feature_mask=seg.expand(2, 100)),
             lambda: fp.attribute(x, target=0, feature_mask=seg), lambda: fp.attribute(x, feature_mask=seg, perturbations_per_eval=0),
             lambda: lime.attribute(x, target=0, feature_mask=seg), lambda: lime.attribute(x, feature_mask=seg, return_input_shape=False),
             lambda: lime.attribute(x, feature_mask=seg, n_samples=0), lambda: lime.attribute(x[0], feature_mask=seg),
             lambda: lime.attribute(x, feature_mask=seg.double()), lambda: lime.attribute(x, feature_mask=seg, baselines=torch.zeros(3, 100)),
             lambda: Lime(_NoEngine(), perturb_func=gen).attribute(x, feature_mask=seg),
             lambda: Lime(_NoEngine(), similarity_func=5).attribute(x, feature_mask=seg),
             lambda: get_exp_kernel_similarity_function("manhattan"), lambda: get_exp_kernel_similarity_function("cosine", 0),
             lambda: get_exp_kernel_similarity_function("euclidean", float("nan")),
             lambda: NoiseTunnel(fp).attribute(x, target=0, feature_mask=seg)]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: fp.attribute(x, feature_mask=seg), lambda: lime.attribute(x, feature_mask=seg - 3),
                 lambda: lime.attribute(x[:1], feature_mask=seg, return_input_shape=False),
                 lambda: NoiseTunnel(lime).attribute(x, feature_mask=seg)):
        with pytest.raises(AssertionError):                                # valid arguments go on to the engine
            call()
    with pytest.raises(TypeError):                                         # any other model has no HIP engine
        Lime(torch.nn.Linear(100, 1)).attribute(x, feature_mask=seg)


def test_captum_names_and_signatures():
    from captum.attr import FeaturePermutation, Lime, NoiseTunnel
    from captum.attr._core.feature_permutation import _permute_feature
    from captum.attr._core.lime import default_perturb_func, get_exp_kernel_similarity_function
    from captum._utils.models.linear_model import SkLearnLasso, SkLearnLinearRegression, SkLearnRidge
    import captum_saliency as cs
    assert (cs.Lime, cs.FeaturePermutation, cs.get_exp_kernel_similarity_function, cs.SkLearnLasso, cs.SkLearnRidge,
            cs.SkLearnLinearRegression) == (Lime, FeaturePermutation, get_exp_kernel_similarity_function, SkLearnLasso, SkLearnRidge,
                                            SkLearnLinearRegression)
    assert list(inspect.signature(Lime.__init__).parameters) == ["self", "forward_func", "interpretable_model", "similarity_func",
                                                                 "perturb_func"]
    p = inspect.signature(Lime.attribute).parameters
    assert list(p) == ["self", "inputs", "baselines", "target", "additional_forward_args", "feature_mask", "n_samples",
                       "perturbations_per_eval", "return_input_shape", "show_progress"]
    assert (p["n_samples"].default, p["perturbations_per_eval"].default, p["return_input_shape"].default) == (50, 1, True)
    p = inspect.signature(FeaturePermutation.__init__).parameters
    assert list(p) == ["self", "forward_func", "perm_func"] and p["perm_func"].default is _permute_feature
    p = inspect.signature(FeaturePermutation.attribute).parameters
    assert list(p) == ["self", "inputs", "target", "additional_forward_args", "feature_mask", "perturbations_per_eval", "show_progress"]
    p = inspect.signature(get_exp_kernel_similarity_function).parameters
    assert (p["distance_mode"].default, p["kernel_width"].default) == ("cosine", 1.0)
    lime = Lime(_NoEngine())
    assert isinstance(lime.interpretable_model, SkLearnLasso) and lime.interpretable_model.alpha == 0.01
    assert lime.perturb_func is default_perturb_func and isinstance(lime.similarity_func, AT.ExpKernelSimilarity)
    assert SkLearnRidge().alpha == 1.0
    z = default_perturb_func(torch.zeros(1, 5), num_interp_features=7)
    assert z.shape == (1, 7) and z.dtype == torch.long and set(z.unique().tolist()) <= {0, 1}
    x = torch.arange(12.0).view(3, 4)
    out = _permute_feature(x, torch.tensor([True, False, False, True]))
    assert torch.equal(out[:, 1:3], x[:, 1:3]) and not torch.equal(out, x)
    NoiseTunnel(lime), NoiseTunnel(FeaturePermutation(_NoEngine()))                 # both wrappable
    p = inspect.signature(cs.explain_waves).parameters
    assert (p["method"].default, p["window"].default, p["stride"].default) == ("input_x_gradient", 1600, 800)
    with pytest.raises(ValueError):                                      # a single clip: before any GPU work
        cs.explain_waves(_NoEngine(), torch.zeros(1, 16000), method="feature_permutation")
    with pytest.raises(ValueError):
        cs.score_explanations(_NoEngine(), torch.zeros(16000), method="feature_permutation")


def test_argument_errors_of_the_lime_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ib = (C.c_int32 * 64)()
    pi = C.addressof(ib)

    def desc(**kw):
        d = dict(x=p, index=pi, perm=pi, n=8, B=2, K=3)
        d.update(kw)
        return AT.PermutationDesc(**d)

    pts = lambda d, row0=0, rows=6, out=p: lib.advh_permutation_points(C.byref(d) if d else None, row0, rows, out, None)
    assert pts(None) == EINVAL
    for bad in (desc(x=None), desc(index=None), desc(perm=None), desc(n=0), desc(B=1), desc(B=0), desc(K=0)):
        assert pts(bad) == EINVAL, bad
    assert pts(desc(), row0=-1) == EINVAL and pts(desc(), rows=-1) == EINVAL and pts(desc(), out=None) == EINVAL
    assert pts(desc(), rows=0) == 0                                        # nothing to write: no launch
    sim = lambda rows_ptr=p, x=p, row0=0, rows=2, B=2, n=8, mode=0, w=1.0, out=p: lib.advh_row_similarity(rows_ptr, x, row0, rows, B, n,
                                                                                                           mode, w, out, None)
    for kw in (dict(rows_ptr=None), dict(x=None), dict(out=None), dict(row0=-1), dict(rows=-1), dict(B=0), dict(n=0), dict(mode=2),
               dict(mode=-1), dict(w=0.0), dict(w=-1.0), dict(w=float("inf")), dict(w=float("nan"))):
        assert sim(**kw) == EINVAL, kw
    assert sim(rows=0) == 0
    X = np.ones(6)
    y = np.ones(3)
    coef = np.zeros(2)
    gap, it = C.c_double(), C.c_int()
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    cd = lambda Xp=dp(X), yp=dp(y), S=3, K=2, alpha=0.1, tol=1e-10, mi=10, cp=dp(coef), g=C.byref(gap), i=C.byref(it): \
        lib.advh_lasso_cd(Xp, yp, S, K, alpha, tol, mi, cp, g, i)
    for kw in (dict(Xp=None), dict(yp=None), dict(cp=None), dict(g=None), dict(i=None), dict(S=0), dict(K=0), dict(alpha=-1.0),
               dict(alpha=float("nan")), dict(alpha=float("inf")), dict(tol=-1.0), dict(tol=float("nan")), dict(mi=0)):
        assert cd(**kw) == EINVAL, kw
    assert cd() == 0 and it.value >= 1


def test_lime_kernels_do_not_spill():
    res = resources("attribution_lime.hip")
    for nm, forms in (("build_rows_kernel", 2), ("row_similarity_kernel", 4)):
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == forms, (nm, sorted(res))                       # float4 and scalar forms (x two distance modes)
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
