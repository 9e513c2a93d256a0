"""CPU-only: the Shapley attributions (ShapleyValueSampling, ShapleyValues, KernelShap): the accumulation order of
csrc/attribution_shapley.hip against the Captum-style restatement of tests/shapley_ref.py, the host draws and the host
regression, argument checking in the engine and the captum.attr front end before any GPU work, the error contract of the entry
points, and their resource usage."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

import shapley_ref as R
from addvisor_hip import _lib, attribution as AT
from test_build_resources import resources


def accumulate_kernel_model(fbase, fk, index, rank, P_div):
    """numpy model of shapley_accumulate_kernel: per sample, float32 sum in increasing p from 0 of
    fk[p, j] - fk[p, j - 1] (fbase for j = 0), j = rank[p][id], then one rounded division."""
    P, K = rank.shape
    B = fbase.shape[0]
    f = fk.reshape(P, K, B)
    L = index.shape[1]
    out = np.empty((B, L), np.float32)
    for b in range(B):
        for t in range(L):
            k = index[0 if index.shape[0] == 1 else b, t]
            acc = np.float32(0)
            for p in range(P):
                j = rank[p, k]
                prev = fbase[b] if j == 0 else f[p, j - 1, b]
                acc = np.float32(acc + np.float32(f[p, j, b] - prev))
            out[b, t] = np.float32(acc / np.float32(P_div))
    return out


@pytest.mark.parametrize("K,P,index_rows", [(3, 25, 1), (5, 7, 3), (8, 40, 1), (4, 24, 3)])
def test_kernel_summation_order_matches_captum_bit_for_bit(K, P, index_rows):
    B, L = 3, 40
    g = torch.Generator().manual_seed(K * 100 + P)
    index = torch.randint(0, K, (index_rows, L), generator=g, dtype=torch.int32)
    rank = AT.shapley_permutations(K + P, P, K)
    perm = np.argsort(rank, axis=1)
    fbase = torch.randn(B, generator=g)
    fk = fbase.repeat(P * K) + 1e-3 * torch.randn(P * K * B, generator=g) * torch.logspace(0, 3, P * K * B)  # three decades
    ref = R.shapley(torch.zeros(B, L), 0.0, index, perm, fbase=fbase, fk=fk)
    ours = accumulate_kernel_model(fbase.numpy(), fk.numpy(), index.numpy(), rank, P)
    assert np.array_equal(ours.view(np.int32), ref.numpy().view(np.int32))


def test_exact_permutations_streamed_in_groups():
    """ShapleyValues' rank tables, drawn in groups, are the ranks of itertools.permutations in order."""
    for K, G in ((1, 1), (3, 4), (4, 5), (5, 7)):
        nxt = AT.exact_permutation_stream(K)
        n = math.factorial(K)
        rank = np.concatenate([nxt(min(G, n - p0)) for p0 in range(0, n, G)])
        assert rank.dtype == np.int32 and rank.shape == (n, K)
        assert np.array_equal(rank, np.argsort(R.all_permutations(K), axis=1))


def test_permutation_draws():
    a = AT.shapley_permutations(11, 500, 6)
    assert a.dtype == np.int32 and a.shape == (500, 6)
    assert np.array_equal(a, AT.shapley_permutations(11, 500, 6))            # reproducible from the seed
    assert not np.array_equal(a, AT.shapley_permutations(12, 500, 6))
    assert np.array_equal(np.sort(a, axis=1), np.tile(np.arange(6), (500, 1)))   # every row is a permutation
    nxt = AT._permutation_stream(11)                                         # groups continue the same stream
    assert np.array_equal(np.concatenate([nxt(7, 6), nxt(493, 6)]), a)
    # uniform: each feature takes each position with probability 1/K (500 draws: 83.3 expected, sd ~8.3)
    counts = np.stack([(a == j).sum(0) for j in range(6)])
    assert np.all(np.abs(counts - 500 / 6) < 5 * np.sqrt(500 * (1 / 6) * (5 / 6))), counts


def test_coalition_draws():
    Ks, S = [2, 5, 12], 4000
    z = AT.kernel_shap_draws(5, Ks, S)
    z2 = AT.kernel_shap_draws(5, Ks, S)
    assert all(np.array_equal(a, b) for a, b in zip(z, z2))                  # reproducible from the seed
    assert not np.array_equal(AT.kernel_shap_draws(6, Ks, S)[2], z[2])
    for K, zb in zip(Ks, z):
        assert zb.dtype == np.uint8 and zb.shape == (S, K) and set(np.unique(zb)) <= {0, 1}
        assert zb[0].all() and not zb[1].any()                              # endpoints first
        k = zb[2:].sum(1)
        assert k.min() >= 1 and k.max() <= K - 1                            # then sizes in [1, K - 1]
        p = AT.kernel_shap_probs(K)
        assert np.isclose(p.sum(), 1) and np.allclose(p * np.arange(1, K) * (K - np.arange(1, K)), p[0] * (K - 1))
        n = S - 2
        freq = np.bincount(k, minlength=K)[1:]
        assert np.all(np.abs(freq - n * p) <= 5 * np.sqrt(n * p * (1 - p)) + 1), (K, freq, n * p)
        if K > 2:                                                           # a uniform subset: each feature in k/K of the rows
            kk = K // 2
            rows = zb[2:][k == kk]
            share = rows.mean(0)
            assert np.all(np.abs(share - kk / K) < 5 * np.sqrt(kk / K * (1 - kk / K) / len(rows))), share
    assert [zb.shape for zb in AT.kernel_shap_draws(5, [3, 4], 2)] == [(2, 3), (2, 4)]


def test_host_solve_matches_independent_weighted_least_squares():
    rng = np.random.default_rng(3)
    for K, S in ((2, 6), (5, 25), (12, 200)):
        z = AT.kernel_shap_draws(K * S, [K], S)[0]
        y = rng.normal(size=S)
        coef, icpt = AT.kernel_shap_fit(z, y)
        w = AT.kernel_shap_weights(z)
        assert np.array_equal(w, R.kernel_weights(z)) and w[0] == w[1] == 1e6 and np.all(w[2:] == 1)
        # independent: the normal equations of [1, z] weighted by w, solved directly
        A = np.hstack([np.ones((S, 1)), z.astype(np.float64)])
        sol = np.linalg.solve(A.T @ (w[:, None] * A), A.T @ (w * y))
        assert np.allclose(coef, sol[1:], rtol=1e-8, atol=1e-8) and np.isclose(icpt, sol[0], rtol=1e-8, atol=1e-8)
        rc, ri = R.linear_regression(z, y, w)
        assert np.allclose(coef, rc, rtol=1e-12, atol=1e-12) and np.isclose(icpt, ri, rtol=1e-12, atol=1e-12)
    # a linear model is recovered exactly: efficiency (intercept = F(empty), intercept + sum = F(full))
    z = AT.kernel_shap_draws(1, [6], 40)[0]
    c = np.array([0.5, -1.0, 2.0, 0.0, 0.25, -0.75])
    coef, icpt = AT.kernel_shap_fit(z, 0.3 + z @ c)
    assert np.allclose(coef, c, atol=1e-9) and np.isclose(icpt, 0.3, atol=1e-9)


def test_feature_indices_for_kernel_shap():
    B, L = 3, 12
    m = torch.tensor([[0, 0, 4, 4, 9, 9] * 2, [5, 5, 5, 5, 5, 6] * 2, [7, 1, 2, 3, 1, 2] * 2])
    index, Ks = AT.kernel_shap_feature_indices(m, B, L)
    assert Ks == [3, 2, 4] and index.dtype == torch.int32
    assert index[0].tolist() == [0, 0, 1, 1, 2, 2] * 2 and index[1].tolist() == [0, 0, 0, 0, 0, 1] * 2
    assert index[2].tolist() == [3, 0, 1, 2, 0, 1] * 2
    index, Ks = AT.kernel_shap_feature_indices(torch.tensor([[3, 3, 8, 8] * 3]), B, L)
    assert Ks == [2, 2, 2] and index.shape == (1, L)
    index, Ks = AT.kernel_shap_feature_indices(None, B, L)
    assert Ks == [L] * B and index.shape == (1, L)
    assert AT.shapley_feature_indices(m, B, L)[1] == 9                       # Shapley: the ids present in the whole mask


def test_engine_validates_before_gpu_work():
    """Argument errors surface before the engine touches the device (the engine object is never used)."""
    att = AT.HipAttribution.__new__(AT.HipAttribution)
    x = torch.zeros(2, 100)
    seg = (torch.arange(100) // 10)[None]
    calls = []
    for name in ("shapley_value_sampling", "shapley_values", "kernel_shap"):
        f = getattr(att, name)
        calls += [lambda f=f: f(x, feature_mask=seg - 1),                             # negative ids
                  lambda f=f: f(x, feature_mask=seg.float()), lambda f=f: f(x, feature_mask=seg.bool()),
                  lambda f=f: f(x, feature_mask=seg[:, :99]), lambda f=f: f(x, feature_mask=torch.zeros(3, 100, dtype=torch.int64)),
                  lambda f=f: f(x, baselines=torch.zeros(3, 100)), lambda f=f: f(x, baselines=torch.zeros(2, 99)),
                  lambda f=f: f(x, baselines=torch.zeros(2, 100, dtype=torch.int64)), lambda f=f: f(x, baselines="zero"),
                  lambda f=f: f(x, feature_mask=seg, internal_batch_size=0), lambda f=f: f(torch.zeros(2, 3, 4))]
    for bad in (0, -1, 2.5, True, None):
        calls += [lambda bad=bad: att.shapley_value_sampling(x, feature_mask=seg, n_samples=bad),
                  lambda bad=bad: att.kernel_shap(x, feature_mask=seg, n_samples=bad)]
    calls += [lambda: att.kernel_shap(x, feature_mask=seg, n_samples=1),                # the regression needs both endpoints
              lambda: att.kernel_shap(x, feature_mask=torch.zeros(1, 100, dtype=torch.int64)),           # K = 1
              lambda: att.kernel_shap(x, feature_mask=torch.stack([seg[0], torch.zeros(100, dtype=torch.int64)])),   # K_1 = 1
              lambda: att.kernel_shap(x, feature_mask=seg, return_input_shape=False),    # B > 1
              lambda: att.shapley_value_sampling(x, feature_mask=seg, seed=-1)]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    with pytest.warns(UserWarning), pytest.raises(AttributeError):                 # warns first, then reaches the (absent) device
        att.shapley_values(x, feature_mask=(torch.arange(100) // 9)[None])


class _NoEngine:
    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.attr import KernelShap, ShapleyValueSampling, ShapleyValues
    x = torch.zeros(2, 100)
    seg = (torch.arange(100) // 10)[None]
    svs, sv, ks = ShapleyValueSampling(_NoEngine()), ShapleyValues(_NoEngine()), KernelShap(_NoEngine())
    calls = []
    for m in (svs, sv, ks):
        calls += [lambda m=m: m.attribute(x, target=0, feature_mask=seg), lambda m=m: m.attribute(x[0], feature_mask=seg),
                  lambda m=m: m.attribute(x, feature_mask=seg - 3), lambda m=m: m.attribute(x, feature_mask=seg.double()),
                  lambda m=m: m.attribute(x, feature_mask=seg, baselines=torch.zeros(3, 100)),
                  lambda m=m: m.attribute(x, feature_mask=seg, perturbations_per_eval=0),
                  lambda m=m: m.attribute(x, feature_mask=seg, perturbations_per_eval=1.5)]
    calls += [lambda: svs.attribute(x, feature_mask=seg, n_samples=0), lambda: ks.attribute(x, feature_mask=seg, n_samples=1),
              lambda: ks.attribute(x, feature_mask=seg, return_input_shape=False),
              lambda: ks.attribute(x, feature_mask=torch.zeros(1, 100, dtype=torch.int64))]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    for call in (lambda: svs.attribute(x, feature_mask=seg, perturbations_per_eval=3), lambda: sv.attribute(x, feature_mask=seg[:, :100] // 5),
                 lambda: ks.attribute(x[:1], feature_mask=seg, return_input_shape=False)):
        with pytest.raises(AssertionError):                          # valid arguments go on to the engine
            call()


def test_captum_names_and_signatures():
    from captum.attr import KernelShap, ShapleyValueSampling, ShapleyValues
    import captum_saliency
    assert (captum_saliency.ShapleyValueSampling, captum_saliency.ShapleyValues, captum_saliency.KernelShap) == \
        (ShapleyValueSampling, ShapleyValues, KernelShap)
    common = ["self", "inputs", "baselines", "target", "additional_forward_args", "feature_mask"]
    p = inspect.signature(ShapleyValueSampling.attribute).parameters
    assert list(p) == common + ["n_samples", "perturbations_per_eval", "show_progress"]
    assert (p["baselines"].default, p["feature_mask"].default, p["n_samples"].default, p["perturbations_per_eval"].default,
            p["show_progress"].default) == (None, None, 25, 1, False)
    p = inspect.signature(ShapleyValues.attribute).parameters
    assert list(p) == common + ["perturbations_per_eval", "show_progress"]
    p = inspect.signature(KernelShap.attribute).parameters
    assert list(p) == common + ["n_samples", "perturbations_per_eval", "return_input_shape", "show_progress"]
    assert (p["n_samples"].default, p["return_input_shape"].default) == (25, True)
    p = inspect.signature(captum_saliency.explain_waves).parameters
    assert (p["method"].default, p["window"].default, p["stride"].default) == ("input_x_gradient", 1600, 800)


def test_argument_errors_of_the_shapley_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ib = (C.c_int32 * 64)()
    pi = C.addressof(ib)
    ub = (C.c_uint8 * 64)()
    pu = C.addressof(ub)

    def desc(**kw):
        d = dict(x=p, base=p, index=pi, rank=pi, present=None, n=8, p0=0, rows=0, B=2, base_rows=1, index_rows=1, mode=0, K=3, P=2)
        d.update(kw)
        return AT.CoalitionDesc(**d)

    pres = dict(mode=1, rank=None, present=pu, rows=6, P=0)
    pts = lambda d, row0=0, rows=6, out=p: lib.advh_coalition_points(C.byref(d) if d else None, row0, rows, out, None)
    acc = lambda d, fb=p, fk=p, p0=0, np_=2, total=p, div=0.0: lib.advh_shapley_accumulate(C.byref(d) if d else None, fb, fk, p0, np_,
                                                                                        total, div, None)
    sca = lambda d, coef=p, attr=p: lib.advh_coalition_scatter(C.byref(d) if d else None, coef, attr, None)
    assert pts(None) == EINVAL and acc(None) == EINVAL and sca(None) == EINVAL
    for bad in (desc(index=None), desc(B=0), desc(n=0), desc(K=0), desc(index_rows=0), desc(index_rows=3), desc(mode=2),
                desc(mode=-1), desc(rank=None), desc(P=-1), desc(p0=-1)):
        assert pts(bad) == EINVAL, bad
        assert acc(bad) == EINVAL, bad
        assert sca(bad) == EINVAL, bad
    for bad in (desc(x=None), desc(base=None), desc(base_rows=0), desc(base_rows=3), desc(**pres, x=None),
                desc(**{**pres, "present": None}), desc(**{**pres, "rows": -1})):
        assert pts(bad) == EINVAL, bad                                     # only the points kernel reads x, base and presence
    assert pts(desc(), rows=-1) == EINVAL and pts(desc(), row0=-1) == EINVAL and pts(desc(), out=None) == EINVAL
    assert pts(desc(p0=3), row0=3 * 3 * 2 - 1, rows=0) == EINVAL             # a row before the table's first permutation
    assert pts(desc(p0=3), row0=3 * 3 * 2, rows=0) == 0 and pts(desc(**pres), rows=0) == 0   # nothing to write: no launch
    assert acc(desc(**pres)) == EINVAL                                       # the accumulation needs rank mode
    assert acc(desc(), fb=None) == EINVAL and acc(desc(), fk=None) == EINVAL and acc(desc(), total=None) == EINVAL
    assert acc(desc(), np_=-1) == EINVAL and acc(desc(), np_=3) == EINVAL and acc(desc(p0=4), p0=3, np_=1) == EINVAL
    assert acc(desc(p0=4), p0=5, np_=2) == EINVAL                            # past the table
    for div in (-1.0, float("inf"), float("nan")):
        assert acc(desc(), div=div) == EINVAL, div
    assert sca(desc(), coef=None) == EINVAL and sca(desc(), attr=None) == EINVAL


def test_shapley_kernels_do_not_spill():
    res = resources("attribution_shapley.hip")
    for nm, forms in (("build_rows_kernel", 2), ("shapley_accumulate_kernel", 1), ("coalition_scatter_kernel", 1)):
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == forms, (nm, sorted(res))                       # float4 and scalar forms of the points kernel
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
