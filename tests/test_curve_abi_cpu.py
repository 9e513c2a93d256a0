"""CPU-only: the error contract of the entry points of csrc/attribution_curve.hip (ADVH_EINVAL before any HIP call, so it can
be exercised without a GPU), and every ValueError path of ``HipAttribution.perturbation_curve`` / ``curve_summary``, of their
mask-domain forms and of ``captum_saliency.evaluate_explanation`` firing before any device call, with CPU tensors in."""
import ctypes as C

import pytest
import torch

from addvisor_hip import _lib, attribution as AT, spectral_attribution as SA

EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def p():
    buf = (C.c_float * 256)()
    yield C.addressof(buf)
    del buf


def test_feature_scores_argument_errors(lib, p):
    f = lib.advh_feature_scores
    assert f(None, p, 1, 2, 8, 4, 0, 0, p, None) == EINVAL
    assert f(p, p, 1, 2, 8, 4, 0, 0, None, None) == EINVAL
    assert f(p, p, 1, 0, 8, 4, 0, 0, p, None) == EINVAL                  # B
    assert f(p, p, 1, 2, 0, 4, 0, 0, p, None) == EINVAL                  # n
    assert f(p, p, 1, 2, 8, 0, 0, 0, p, None) == EINVAL                  # K
    assert f(p, p, 1, 2, 8, 9, 0, 0, p, None) == EINVAL                  # K > n
    assert f(p, p, 3, 2, 8, 4, 0, 0, p, None) == EINVAL                  # index_rows not in {1, B}
    assert f(p, p, 0, 2, 8, 4, 0, 0, p, None) == EINVAL
    assert f(p, None, 0, 2, 8, 4, 0, 0, p, None) == EINVAL               # the identity needs K == n


def test_feature_rank_argument_errors(lib, p):
    f = lib.advh_feature_rank
    assert f(None, 2, 4, 1, p, None) == EINVAL
    assert f(p, 2, 4, 1, None, None) == EINVAL
    assert f(p, 0, 4, 1, p, None) == EINVAL
    assert f(p, 2, 0, 0, p, None) == EINVAL
    assert f(p, -1, 4, 0, p, None) == EINVAL


def desc(p, **kw):
    d = AT.CurveDesc(p, p, p, p, p, 8, 2, 1, 1, 4, 3, 0)                 # x, base, index, rank, counts, n, B, base_rows, index_rows, K, S1, mode
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_curve_points_argument_errors(lib, p):
    f = lib.advh_curve_points
    assert f(None, 0, 1, p, None) == EINVAL
    assert f(C.byref(desc(p)), 0, 1, None, None) == EINVAL
    for field in ("x", "base", "rank", "counts"):
        assert f(C.byref(desc(p, **{field: None})), 0, 1, p, None) == EINVAL, field
    for kw in (dict(n=0), dict(B=0), dict(K=0), dict(K=9), dict(base_rows=3), dict(base_rows=0), dict(index_rows=3), dict(mode=2),
               dict(mode=-1), dict(S1=0), dict(S1=6), dict(index=None)):     # S1 = 6 counts cannot increase strictly inside [0, 4]
        assert f(C.byref(desc(p, **kw)), 0, 1, p, None) == EINVAL, kw
    assert f(C.byref(desc(p)), -1, 1, p, None) == EINVAL
    assert f(C.byref(desc(p)), 0, -1, p, None) == EINVAL
    assert f(C.byref(desc(p)), 0, 0, p, None) == 0                       # rows == 0 launches nothing
    assert f(C.byref(desc(p, index=None, K=8)), 0, 0, p, None) == 0      # the identity: K == n


def test_curve_fold_argument_errors(lib, p):
    f = lib.advh_curve_fold
    ok = [p, p, 2, 3, 4, 1, 0, p, p, p, None]
    for i in (0, 1, 7, 8, 9):
        args = list(ok)
        args[i] = None
        assert f(*args) == EINVAL, i
    for i, v in ((2, 0), (3, 1), (3, 0), (3, 6), (4, 0)):                # B, S1 < 2, S1 > K + 1, K
        args = list(ok)
        args[i] = v
        assert f(*args) == EINVAL, (i, v)


class _NoDevice:
    """Stands in for the engine's embedder: any touch of the device fails the test."""
    @property
    def dev(self):
        raise AssertionError("a device call before the argument checks finished")


def engine():
    att = AT.HipAttribution.__new__(AT.HipAttribution)
    att.emb = _NoDevice()
    return att


def wave_cases():
    B, L = 2, 64
    x, a = torch.randn(B, L), torch.randn(B, L)
    seg = (torch.arange(L) // 8)[None]
    gap = torch.stack([seg[0], seg[0].clamp(max=6)])                     # clip 1 holds no sample of feature 7
    return x, a, seg, [
        dict(mode="removal"), dict(order="best"), dict(output="probability"), dict(pool="max"), dict(use_abs=1),
        dict(steps=0), dict(steps=9, feature_mask=seg), dict(steps=[0.0, 0.5]), dict(steps=[0.0, 0.01, 1.0], feature_mask=seg),
        dict(steps=2.0), dict(feature_mask=seg.float()), dict(feature_mask=seg[:, :10]), dict(feature_mask=-seg),
        dict(feature_mask=gap), dict(baselines=torch.zeros(3, L)), dict(baselines="zero"), dict(internal_batch_size=0),
        dict(order="random", seed=-1), dict(order="random", seed=2 ** 64),
    ]


def test_perturbation_curve_value_errors_fire_before_any_device_call():
    att = engine()
    x, a, seg, cases = wave_cases()
    for kw in cases:
        with pytest.raises(ValueError):
            att.perturbation_curve(x, a, **kw)
    for bad in (a[:, :10], a[:1], a.long(), a.numpy(), None):
        with pytest.raises(ValueError):
            att.perturbation_curve(x, bad)
    with pytest.raises(ValueError):
        att.perturbation_curve(x[None], a)
    for kw in cases:
        if not {"mode", "order", "output", "seed"} & set(kw):
            with pytest.raises(ValueError):
                att.curve_summary(x, a, **kw)
    # valid arguments get past the checks and only then reach for the device
    with pytest.raises(AssertionError, match="device call"):
        att.perturbation_curve(x, a, feature_mask=seg, steps=4)


def test_mask_domain_value_errors_fire_before_any_device_call():
    eng = SA.HipSpectralAttribution.__new__(SA.HipSpectralAttribution)
    eng.B, eng.T = 2, 10
    eng._rows = SA._MaskRows.__new__(SA._MaskRows)
    eng._rows.emb = _NoDevice()
    m, a = torch.rand(2, 16, 8), torch.randn(2, 16, 8)
    ids = SA.tf_feature_mask(16, 8, 4, 4)
    for args, kw in (((m, a[:, :, :4]), {}), ((m, a.reshape(2, -1)), {}), ((m[:1], a[:1]), {}), ((m, a), dict(feature_mask=ids[:, :8])),
                     ((m, a), dict(baselines=torch.zeros(1, 16, 4))), ((m, a), dict(feature_mask=ids, steps=9)),
                     ((m, a), dict(feature_mask=ids, mode="both")), ((torch.rand(2, 16, 11), torch.rand(2, 16, 11)), {})):
        with pytest.raises(ValueError):
            eng.perturbation_curve(*args, **kw)
    with pytest.raises(ValueError):
        eng.curve_summary(m, a, feature_mask=ids, pool="median")
    with pytest.raises(AssertionError, match="device call"):
        eng.curve_summary(m, a, feature_mask=ids, baselines=0.5)
    with pytest.raises(NotImplementedError):
        eng.kernel_shap(m)


def test_evaluate_explanation_value_errors():
    import captum_saliency as cs
    x, a = torch.randn(2, 64), torch.randn(2, 64)
    for kw in (dict(domain="mel"), dict(segment=0), dict(segment=1.5), dict(mask=torch.ones(2, 4, 4))):
        with pytest.raises(ValueError):
            cs.evaluate_explanation(None, x, a, **kw)
    with pytest.raises(ValueError):
        cs.evaluate_explanation(None, x[0], a)
    with pytest.raises(ValueError):
        cs.evaluate_explanation(None, x, a, domain="spectrogram")       # a [B, L] map is not a [B, Fm, Tm] one
