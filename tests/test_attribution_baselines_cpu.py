"""CPU-only: the public API, the host-side tables / draws / validation and the argument contract of the baseline-aware
attribution entry points (csrc/attribution_paths.hip)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import attribution_baselines_ref as R
from addvisor_hip import _lib, attribution as AT
from test_build_resources import resources


def test_captum_names_and_signatures():
    from captum.attr import GradientShap, IntegratedGradients
    import captum_saliency
    assert captum_saliency.GradientShap is GradientShap                  # reference line 3 imports all four names
    p = inspect.signature(GradientShap.attribute).parameters
    assert list(p) == ["self", "inputs", "baselines", "n_samples", "stdevs", "target", "additional_forward_args",
                       "return_convergence_delta"]
    assert p["baselines"].default is inspect.Parameter.empty
    assert (p["n_samples"].default, p["stdevs"].default, p["target"].default, p["additional_forward_args"].default,
            p["return_convergence_delta"].default) == (5, 0.0, None, None, False)
    assert inspect.signature(GradientShap.__init__).parameters["multiply_by_inputs"].default is True
    ig = inspect.signature(IntegratedGradients.attribute).parameters
    assert (ig["baselines"].default, ig["method"].default, ig["return_convergence_delta"].default) == (None, "gausslegendre", False)
    IntegratedGradients(object(), multiply_by_inputs=False)             # accepted now (was NotImplementedError)


@pytest.mark.parametrize("n", [2, 4, 50])
@pytest.mark.parametrize("method", AT.METHODS)
def test_approximation_tables(method, n):
    a, w = AT.approximation(method, n)
    ra, rw = R.approximation(method, n)
    assert a.shape == w.shape == (n,)
    np.testing.assert_allclose(a, ra, rtol=0, atol=1e-15)
    np.testing.assert_allclose(w, rw, rtol=0, atol=1e-15)
    if method.startswith("riemann"):
        assert np.all(w[1:-1] == 1.0 / n)
    if method == "riemann_trapezoid":
        assert a[0] == 0 and a[-1] == 1 and w[0] == w[-1] == 0.5 / n
    if method == "riemann_left":
        assert a[0] == 0 and np.isclose(a[-1], 1 - 1 / n)
    if method == "riemann_right":
        assert np.isclose(a[0], 1 / n) and a[-1] == 1
    if method == "riemann_middle":
        assert np.isclose(a[0], 1 / (2 * n)) and np.isclose(a[-1], 1 - 1 / (2 * n))
    if method == "gausslegendre":
        assert np.isclose(w.sum(), 1.0) and np.all((a > 0) & (a < 1))


def test_approximation_rejects():
    with pytest.raises(ValueError):
        AT.approximation("riemann_left", 1)
    with pytest.raises(ValueError):
        AT.approximation("simpson", 8)


def test_shap_draws():
    i1, a1 = AT.shap_draws(123, 3, 5, 4)
    i2, a2 = AT.shap_draws(123, 3, 5, 4)
    assert np.array_equal(i1, i2) and np.array_equal(a1, a2)
    assert i1.shape == a1.shape == (15,) and i1.dtype == np.int32 and a1.dtype == np.float32
    assert i1.min() >= 0 and i1.max() < 4 and a1.min() >= 0 and a1.max() < 1
    i3, a3 = AT.shap_draws(124, 3, 5, 4)
    assert not np.array_equal(a1, a3)
    big_i, big_a = AT.shap_draws(7, 64, 64, 3)
    assert set(np.unique(big_i)) == {0, 1, 2} and 0.45 < big_a.mean() < 0.55
    # the stated stream: B * S indices, then B * S coefficients, entry b * S + s for clip b, sample s
    rng = np.random.Generator(np.random.PCG64(123))
    ri = rng.integers(0, 4, size=15, dtype=np.int32)
    ra = rng.random(15, dtype=np.float32)
    assert np.array_equal(ri, i1) and np.array_equal(ra, a1)
    torch.manual_seed(5)
    s1 = AT.draw_seed()
    torch.manual_seed(5)
    assert AT.draw_seed() == s1 and 0 <= s1 < 2 ** 63


def test_baseline_validation():
    B, L = 2, 100
    for bad in (torch.zeros(B + 1, L), torch.zeros(B, L - 1), torch.zeros(L), torch.zeros(B, L, dtype=torch.int32)):
        with pytest.raises(ValueError):
            AT.check_ig_baselines(bad, B, L)
    assert AT.check_ig_baselines(None, B, L).shape == (1, L) and AT.check_ig_baselines(0.5, B, L)[0, 3] == 0.5
    assert AT.check_ig_baselines(torch.ones(1, L), B, L).shape == (1, L)
    for bad in (torch.zeros(3, L - 1), torch.zeros(L), torch.zeros(3, L, dtype=torch.int64), np.zeros((3, L))):
        with pytest.raises(ValueError):
            AT.check_shap_args(bad, B, L, 5, 0.0)
    with pytest.raises(ValueError):
        AT.check_shap_args(torch.zeros(3, L), B, L, 0, 0.0)
    with pytest.raises(ValueError):
        AT.check_shap_args(torch.zeros(3, L), B, L, 5, -0.1)
    assert AT.check_shap_args(torch.zeros(3, L), B, L, 5, 0.1).shape == (3, L)


def test_engine_validates_before_gpu_work():
    """Argument errors surface before the engine touches the device (the engine object is never used)."""
    att = AT.HipAttribution.__new__(AT.HipAttribution)
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError):
        att.integrated_gradients(x, baselines=torch.zeros(3, 100))
    with pytest.raises(ValueError):
        att.integrated_gradients(x, baselines=torch.zeros(2, 100), method="riemann_left", n_steps=1)
    with pytest.raises(NotImplementedError):
        att.integrated_gradients(x, baselines=0.1, multiply_by_inputs=False, return_convergence_delta=True)
    with pytest.raises(ValueError):
        att.gradient_shap(x, torch.zeros(3, 99))
    with pytest.raises(ValueError):
        att.gradient_shap(x, lambda: torch.zeros(3, 100), stdevs=-1.0)


def test_philox_known_answers():
    """The numpy restatement the GPU test compares the device words with: Random123's Philox4x32-10 known-answer vectors."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, out in kat:
        assert tuple(int(v) for v in R.philox4x32_10(np.array([ctr], np.uint32), *key)[0]) == out


def test_argument_errors_of_the_path_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched) for the baseline-aware attribution entry
    points: validation happens before any HIP call, so it runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ib = (C.c_int32 * 64)()
    pi = C.addressof(ib)

    def desc(**kw):
        d = dict(x=p, base=p, bidx=None, n=8, seed=1, B=2, S=4, base_rows=2, clip_major=0, sigma=0.0)
        d.update(kw)
        return AT.PathDesc(**d)

    ok = desc()
    pts = lambda d, row0=0, rows=8, alpha=p, out=p: lib.advh_attr_path_points(C.byref(d) if d else None, alpha, row0, rows, out, None)
    acc = lambda d, mode, row0=0, rows=8, w=p, total=p, rs=None, grad=p: lib.advh_attr_path_accumulate(
        C.byref(d), grad, w, mode, row0, rows, total, rs, None)
    assert pts(None) == EINVAL
    for bad in (desc(x=None), desc(base=None), desc(B=0), desc(S=0), desc(n=0), desc(n=-4), desc(base_rows=3),
                desc(base_rows=0), desc(sigma=-1.0), desc(sigma=float("inf")), desc(sigma=float("nan")), desc(clip_major=2)):
        assert pts(bad) == EINVAL
        assert acc(bad, 0) == EINVAL
    assert pts(ok, rows=0) == EINVAL and pts(ok, rows=-1) == EINVAL
    assert pts(ok, row0=-1) == EINVAL
    assert pts(ok, row0=1, rows=8) == EINVAL                              # past B * S rows
    assert pts(ok, alpha=None) == EINVAL and pts(ok, out=None) == EINVAL
    assert acc(ok, 0, grad=None) == EINVAL and acc(ok, 0, total=None) == EINVAL
    assert acc(ok, 0, w=None) == EINVAL                                   # IG needs weights
    assert acc(ok, 0, rs=p) == EINVAL                                     # no row sums in IG chunks
    assert acc(ok, 1) == EINVAL                                           # GradientShap rows are clip-major
    assert acc(ok, 5) == EINVAL and acc(ok, -1) == EINVAL
    assert acc(ok, 0, rows=9) == EINVAL and acc(ok, 0, rows=0) == EINVAL
    shap = desc(bidx=pi, base_rows=3, clip_major=1)
    assert acc(shap, 1, row0=4, rows=5) == EINVAL
    assert acc(shap, 0) == EINVAL                                         # IG rows are step-major
    assert acc(ok, 3, rows=4) == EINVAL and acc(ok, 3, row0=2, rows=2) == EINVAL   # finalize: rows = B from 0
    assert acc(shap, 3, rows=2) == EINVAL                                 # IG finalize has no gathered baselines
    assert acc(shap, 4, rows=2, rs=p) == EINVAL                           # no sums of the mean
    assert lib.advh_philox_normal(1, 0, 4, 8, 0, None, None) == EINVAL
    assert lib.advh_philox_normal(1, -1, 4, 8, 0, p, None) == EINVAL
    assert lib.advh_philox_normal(1, 0, 0, 8, 0, p, None) == EINVAL
    assert lib.advh_philox_normal(1, 0, 4, 0, 0, p, None) == EINVAL
    assert lib.advh_philox_normal(1, 0, 4, 8, 2, p, None) == EINVAL


def test_path_kernels_do_not_spill():
    res = resources("attribution_paths.hip")
    names = ("path_points_kernel", "path_accumulate_kernel", "path_finalize_kernel", "path_row_sum_kernel", "philox_normal_kernel")
    for nm in names:
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == 2, (nm, sorted(res))                           # float4 and scalar forms
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
