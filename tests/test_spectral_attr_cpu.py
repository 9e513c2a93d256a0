"""CPU-only: the host side of the time-frequency attributions (addvisor_hip/spectral_attribution.py, the captum.attr front end
over ``captum_saliency.MaskedSpectrogramLogReg``): the 2-D occlusion's window enumeration and coverage counts against the
numpy restatement of tests/spectral_attr_ref.py, ``tf_feature_mask``, every ValueError / NotImplementedError of the front end
before an engine exists, and the argument errors of the new entry points (negative codes, nothing launched)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectral_attr_ref as R
from addvisor_hip import _lib
from addvisor_hip import spectral_attribution as SA

CASES = [((3, 2), (2, 1)), ((3, 2), (3, 2)), ((7, 5), (1, 1)), ((7, 5), (7, 5))]        # the last two: a window equal to the input


@pytest.mark.parametrize("window,stride", CASES)
def test_window_enumeration_and_coverage(window, stride):
    Fm, Tm = 7, 5
    masks = R.occlusion2d_masks(Fm, Tm, window, stride)
    w, s, (Kf, Kt) = SA.check_occlusion2d_args(Fm, Tm, window, stride)
    assert (Kf, Kt) == R.occlusion2d_shifts(Fm, Tm, window, stride) and Kf * Kt == masks.shape[0]
    fl, fh, tl, th = R.occlusion2d_cover(Fm, Tm, w, s)
    counts = np.outer(fh - fl + 1, th - tl + 1)
    assert np.array_equal(counts, masks.sum(0).astype(np.int64)) and counts.min() >= 1
    for f in range(Fm):                                                  # the windows themselves, k = kf * Kt + kt
        for t in range(Tm):
            ks = sorted(kf * Kt + kt for kf in range(fl[f], fh[f] + 1) for kt in range(tl[t], th[t] + 1))
            assert ks == list(np.nonzero(masks[:, f, t])[0]), (f, t)
    if window != (Fm, Tm):
        assert masks[-1].sum() <= window[0] * window[1]                  # the last window is cropped at the edges, never wrapped


def test_occlusion2d_argument_errors():
    for window, stride in (((3,), (1, 1)), (3, (1, 1)), ((8, 2), None), ((3, 6), None), ((3, 2), (4, 1)), ((3, 2), (1, 3)),
                           ((0, 2), None), ((3, 2), (1,)), ((3.0, 2), None)):
        with pytest.raises(ValueError):
            SA.check_occlusion2d_args(7, 5, window, stride)
    assert SA.check_occlusion2d_args(7, 5, (7, 2), (9, 1))[2] == (1, 4)     # a stride past a window that spans the axis is allowed


def test_tf_feature_mask_ids():
    import captum_saliency as CS
    m = CS.tf_feature_mask(513, 50, 64, 16)
    assert m.shape == (1, 513, 50) and m.dtype == torch.int64
    f, t = torch.arange(513)[:, None], torch.arange(50)[None, :]
    assert torch.equal(m[0], (f // 64) * 4 + t // 16)
    assert int(m.max()) == 8 * 4 + 3 and m.unique().numel() == 36       # bin 512 is a band of its own
    bands = CS.tf_feature_mask(512, 48)                                  # one feature per 1 kHz band
    assert torch.equal(bands[0], (torch.arange(512) // 64)[:, None].expand(512, 48)) and bands.unique().numel() == 8
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            CS.tf_feature_mask(*bad)
    with pytest.raises(ValueError):
        CS.tf_feature_mask(4, 4, 0)


class _NoEngine:
    """A mask-domain model whose engine must never be asked for: the front end's checks come first."""
    def hip_mask_attribution(self):
        raise AssertionError("the engine was created before the arguments were checked")

    def mask_frames(self):
        return 50

    def num_clips(self):
        return 2


def test_front_end_errors_fire_before_the_engine():
    import captum.attr as CA
    import captum.metrics as CM
    import captum.robust as CR
    m = _NoEngine()
    x = torch.ones(2, 512, 48)
    ids = torch.zeros(1, 512, 48, dtype=torch.long)
    bad_inputs = [torch.ones(2, 16000), torch.ones(2, 514, 48), torch.ones(2, 512, 51), torch.ones(3, 512, 48),
                  torch.ones(2, 512, 48, dtype=torch.long), "x"]
    for cls in (CA.Saliency, CA.InputXGradient, CA.IntegratedGradients, CA.FeatureAblation, CA.ShapleyValueSampling):
        for bad in bad_inputs:
            with pytest.raises(ValueError):
                cls(m).attribute(bad)
        with pytest.raises(ValueError):
            cls(m).attribute(x, target=1)
    for bad in bad_inputs:
        with pytest.raises(ValueError):
            CA.GradientShap(m).attribute(bad, torch.ones(3, 512, 48))
        with pytest.raises(ValueError):
            CA.Occlusion(m).attribute(bad, (64, 8))
    ig = CA.IntegratedGradients(m)
    for kw in ({"baselines": torch.ones(2, 512, 47)}, {"baselines": torch.ones(3, 512, 48)}, {"baselines": torch.ones(2, 512 * 48)},
               {"baselines": ids}, {"method": "simpson"}, {"n_steps": 0}, {"n_steps": 1, "method": "riemann_trapezoid"},
               {"internal_batch_size": 0}):
        with pytest.raises(ValueError):
            ig.attribute(x, **kw)
    gs = CA.GradientShap(m)
    for args, kw in (((torch.ones(512, 48),), {}), ((torch.ones(2, 512, 47),), {}), ((ids,), {}),
                     ((torch.ones(1, 512, 48),), {"n_samples": 0}), ((torch.ones(1, 512, 48),), {"stdevs": -1.0})):
        with pytest.raises(ValueError):
            gs.attribute(x, *args, **kw)
    with pytest.raises(NotImplementedError):
        gs.attribute(x, torch.ones(1, 512, 48), return_convergence_delta=True)
    with pytest.raises(NotImplementedError):
        gs.attribute(x, lambda: torch.ones(1, 512, 48))
    oc = CA.Occlusion(m)
    for args, kw in ((((64,),), {}), ((1600,), {}), (((513, 8),), {}), (((64, 49),), {}), (((64, 8),), {"strides": (65, 4)}),
                     (((64, 8),), {"strides": 4}), (((64, 8),), {"baselines": torch.ones(2, 16000)}),
                     (((64, 8),), {"perturbations_per_eval": 0}), (((64, 8),), {"target": 0})):
        with pytest.raises(ValueError):
            oc.attribute(x, *args, **kw)
    for cls in (CA.FeatureAblation, CA.ShapleyValueSampling):
        for kw in ({"feature_mask": torch.zeros(1, 512 * 48, dtype=torch.long)}, {"feature_mask": torch.zeros(1, 512, 48)},
                   {"feature_mask": torch.zeros(3, 512, 48, dtype=torch.long)}, {"baselines": torch.ones(1, 512, 47)},
                   {"perturbations_per_eval": 0}):
            with pytest.raises(ValueError):
                cls(m).attribute(x, **kw)
    with pytest.raises(ValueError):
        CA.ShapleyValueSampling(m).attribute(x, feature_mask=ids - 1)          # Shapley ids are >= 0
    with pytest.raises(ValueError):
        CA.ShapleyValueSampling(m).attribute(x, feature_mask=ids, n_samples=0)
    # not in the mask-domain engine: NotImplementedError that names it
    for make in (lambda: CA.KernelShap(m).attribute(x), lambda: CA.Lime(m).attribute(x), lambda: CA.ShapleyValues(m).attribute(x),
                 lambda: CA.FeaturePermutation(m).attribute(x), lambda: CA.NoiseTunnel(CA.Saliency(m)).attribute(x),
                 lambda: CA.LayerActivation(m, 0).attribute(x), lambda: CA.NeuronGradient(m, 0).attribute(x, (0, 0)),
                 lambda: CM.infidelity(m, lambda v: (v, v), x, x), lambda: CR.FGSM(m).perturb(x, 0.1, 0),
                 lambda: CR.PGD(m).perturb(x, 0.1, 0.01, 2, 0)):
        with pytest.raises(NotImplementedError, match="HipSpectralAttribution"):
            make()


def test_engine_names_what_it_does_not_implement():
    for name in ("kernel_shap", "lime", "feature_permutation", "noise_tunnel", "infidelity", "sensitivity_max"):
        with pytest.raises(NotImplementedError, match="HipSpectralAttribution"):
            getattr(SA.HipSpectralAttribution, name)(None)


def test_models_without_the_attribute_take_todays_path():
    """A 3-D input to a waveform model still raises what it raised: the branch is taken on the model, not on the input."""
    import captum.attr as CA

    class Wave:
        def hip_attribution(self):
            raise AssertionError("no engine for a bad input")
    x = torch.ones(2, 512, 48)
    with pytest.raises(ValueError, match=r"\[B, L\] waveform"):
        CA.Saliency(Wave()).attribute(x)
    with pytest.raises(ValueError, match=r"\[B, L\] waveform"):
        CA.Occlusion(Wave()).attribute(x, (64, 8))
    with pytest.raises(ValueError):
        CA.Occlusion(Wave()).attribute(torch.ones(2, 1600), (64, 8))           # a 2-tuple is not a waveform window
    with pytest.raises(TypeError):
        CA.Saliency(object()).attribute(torch.ones(2, 1600))


def test_masked_model_checks_its_arguments():
    import captum_saliency as CS

    class Wave:
        def hip_attribution(self):
            raise AssertionError("no engine at construction")
    with pytest.raises(TypeError):
        CS.MaskedSpectrogramLogReg(object(), torch.ones(2, 16000))
    with pytest.raises(ValueError):
        CS.MaskedSpectrogramLogReg(Wave(), torch.ones(2, 16000), domain="db")
    with pytest.raises(ValueError):
        CS.MaskedSpectrogramLogReg(Wave(), torch.ones(2, 3, 16000))
    mm = CS.MaskedSpectrogramLogReg(Wave(), torch.ones(2, 16000))
    assert mm.mask_frames() == 50 and mm.num_clips() == 2
    with pytest.raises(ValueError):
        CS.explain_spectrogram(Wave(), torch.ones(2, 16000), method="lime")


def test_new_entry_points_reject_bad_arguments():
    """Negative return codes before any HIP call (no device is initialised in this process)."""
    lib = _lib.lib()
    EINVAL = -1
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    B, T, L = 2, 50, 16000

    def rows(spec=p, mask=p, Fm=512, Tm=48, mode=1, wave=p, stride=L, rows=5, row0=0, cm=0, S=1, B=B, T=T):
        return lib.advh_istft_masked_rows(spec, mask, Fm, Tm, mode, wave, stride, rows, row0, cm, S, B, T, L, 322, 644, None, None)

    def rows_bwd(g=p, spec=p, mask=p, Fm=512, Tm=48, mode=1, dmask=p, stride=L, rows=5, row0=0, cm=0, S=1, B=B, T=T):
        return lib.advh_istft_masked_rows_bwd(g, stride, spec, mask, Fm, Tm, mode, dmask, rows, row0, cm, S, B, T, L, 322, 644, None,
                                              None)
    for fn in (rows, rows_bwd):
        assert fn() < 0                                                  # valid arguments, but no device initialised: ENOTINIT
        for kw in ({"rows": 0}, {"rows": -1}, {"Fm": 514}, {"Fm": 0}, {"Tm": T + 1}, {"Tm": 0}, {"S": 0}, {"S": -3}, {"spec": None},
                   {"row0": -1}, {"cm": 2}, {"B": 0}, {"mode": 0}, {"mode": 3}, {"stride": L - 1}):
            assert fn(**kw) == EINVAL, kw
    assert rows(mask=None) == EINVAL and rows(wave=None) == EINVAL
    assert rows_bwd(g=None) == EINVAL and rows_bwd(dmask=None) == EINVAL
    assert rows_bwd(mask=None, mode=2) == EINVAL                         # the log1p adjoint reads the mask
    assert rows_bwd(mask=None, mode=1) != EINVAL                         # the linear one does not

    d = SA.Occlusion2dDesc(p, p, 2, 1, 7, 5, 3, 2, 2, 1, 3, 4)
    assert lib.advh_occlusion2d_points(C.byref(d), 0, 0, p, None) == 0    # rows = 0 launches nothing
    assert lib.advh_occlusion2d_points(None, 0, 1, p, None) == EINVAL
    assert lib.advh_occlusion2d_points(C.byref(d), 0, 1, None, None) == EINVAL
    assert lib.advh_occlusion2d_points(C.byref(d), -1, 1, p, None) == EINVAL
    assert lib.advh_occlusion2d_points(C.byref(d), 0, -1, p, None) == EINVAL
    assert lib.advh_occlusion2d_accumulate(C.byref(d), None, p, p, None) == EINVAL
    for field, v in (("Kf", 4), ("Kt", 3), ("wf", 8), ("wt", 0), ("sf", 4), ("st", 3), ("B", 0), ("base_rows", 3), ("x", None),
                     ("base", None)):
        bad = SA.Occlusion2dDesc(p, p, 2, 1, 7, 5, 3, 2, 2, 1, 3, 4)
        setattr(bad, field, v)
        assert lib.advh_occlusion2d_points(C.byref(bad), 0, 1, p, None) == EINVAL, field
        assert lib.advh_occlusion2d_accumulate(C.byref(bad), p, p, p, None) == EINVAL, field
    for args in ((None, 2, 7, 5, 3, 2, p), (p, 2, 7, 5, 3, 2, None), (p, 0, 7, 5, 3, 2, p), (p, 2, 0, 5, 3, 2, p), (p, 2, 7, 0, 3, 2, p),
                 (p, 2, 7, 5, 0, 2, p), (p, 2, 7, 5, 3, 0, p)):
        assert lib.advh_tf_pool(*args, None) == EINVAL, args
