"""CPU-only: the neuron attributions' selector check, every argument check of the captum.attr neuron classes and of the engine
runs before any GPU work, the two entry points of csrc/attribution_neuron.hip keep the header's error contract and compile
without scratch, and the restatement (tests/neuron_attr_ref.py) is consistent with itself: selection by plain indexing, the
fp32-versus-fp64 gradient and the quadrature error of NeuronIntegratedGradients (printed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import neuron_attr_ref as NR
from addvisor_hip import _lib, attribution as AT, synthetic as syn
from addvisor_hip.embedder_grad import check_box
from test_build_resources import resources

torch.set_grad_enabled(False)
T, H = 49, 64
BAND = (slice(0, 49, 2), slice(60, 64))


def noise_baseline(B, L, seed=3):
    return 0.05 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def model_of(cfg):
    return (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))


@pytest.fixture(scope="module", params=[False, True], ids=["post_ln", "pre_ln"])
def model(request):
    return model_of(syn.tiny_config(request.param))


def test_check_neuron_selector_table():
    ok = [((7, 5), (7, 8, 1, 5, 6, 1)), ((0, 0), (0, 1, 1, 0, 1, 1)), ((48, 63), (48, 49, 1, 63, 64, 1)),
          ((-1, -1), (48, 49, 1, 63, 64, 1)), ((-49, -64), (0, 1, 1, 0, 1, 1)), ((np.int64(3), np.int32(-2)), (3, 4, 1, 62, 63, 1)),
          (BAND, (0, 49, 2, 60, 64, 1)), ((slice(None), 5), (0, 49, 1, 5, 6, 1)),
          ((slice(None, None, 3), slice(1, None, 7)), (0, 49, 3, 1, 64, 7)), ((slice(-4, None), slice(-8, -4)), (45, 49, 1, 56, 60, 1)),
          ((slice(10, 1000), slice(-1000, 3)), (10, 49, 1, 0, 3, 1)), ((slice(5, 6), slice(2, 4, 2)), (5, 6, 1, 2, 4, 2))]
    for sel, box in ok:
        assert AT.check_neuron_selector(sel, T, H) == box, sel
        assert AT.check_neuron_selector(list(sel), T, H) == box
        assert check_box(box, T, H) == box
        # the box selects what Python's indexing selects
        idx = torch.arange(T * H).view(1, T, H).double()
        t0, t1, ts, h0, h1, hs = box
        assert NR.select(idx, sel).item() == idx[0, t0:t1:ts, h0:h1:hs].sum().item(), sel
    bad = (5, (5,), (1, 2, 3), None, "ab", (49, 0), (0, 64), (-50, 0), (0, -65), (1.0, 2), (True, 2), ("1", 2), (None, 2),
           (slice(0, 10, 0), 1), (slice(0, 10, -1), 1), (slice(10, 0, -1), 1), (slice(5, 5), 1), (slice(49, None), 1), (1, slice(64, 70)),
           (slice(0.0, 3), 1), (1, slice(0, 4, 1.0)), (torch.tensor(1), 2), ([1, 2], 3))
    for sel in bad:
        with pytest.raises(ValueError):
            AT.check_neuron_selector(sel, T, H)
    for sel in (lambda h: h[:, 0, 0], torch.sum):
        with pytest.raises(NotImplementedError):
            AT.check_neuron_selector(sel, T, H)
    for box in ((0, 0, 1, 0, 1, 1), (0, 50, 1, 0, 1, 1), (0, 1, 0, 0, 1, 1), (0, 1, 1, 0, 65, 1), (-1, 1, 1, 0, 1, 1), (0, 1, 1, 0, 1),
                (0, 1, 1, 0, 1, 1.0), None, (slice(0, 1), 0)):
        with pytest.raises(ValueError):
            check_box(box, T, H)


class _NoEngine:
    def num_layers(self):
        return 9

    def frame_shape(self, n):
        return T, H

    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.attr import (NeuronConductance, NeuronFeatureAblation, NeuronGradient, NeuronGradientShap, NeuronIntegratedGradients,
                             NoiseTunnel)
    import captum_saliency
    for name in ("NeuronGradient", "NeuronIntegratedGradients", "NeuronGradientShap", "NeuronConductance", "NeuronFeatureAblation"):
        assert getattr(captum_saliency, name) is getattr(__import__("captum.attr", fromlist=[name]), name)
    x = torch.zeros(2, 100)
    m = _NoEngine()
    shap = lambda cls: {"baselines": torch.zeros(3, 100)} if cls is NeuronGradientShap else {}
    classes = (NeuronGradient, NeuronIntegratedGradients, NeuronGradientShap, NeuronConductance, NeuronFeatureAblation)
    for cls in classes:
        kw = shap(cls)
        for bad in (-1, 10, 2.0, "4", None, True):                        # a layer out of range or not an int
            with pytest.raises(ValueError):
                cls(m, bad).attribute(x, (7, 5), **kw)
        for bad in (5, (5,), (1, 2, 3), (49, 0), (0, -65), (slice(0, 4, 0), 1), (slice(4, 4), 1), (1.5, 2)):
            with pytest.raises(ValueError):
                cls(m, 4).attribute(x, bad, **kw)
        with pytest.raises(NotImplementedError):
            cls(m, 4).attribute(x, lambda h: h[:, 0, 0], **kw)
        with pytest.raises(ValueError):
            cls(m, 4).attribute(x[0], (7, 5), **kw)
        with pytest.raises(NotImplementedError):
            cls(m, 4).attribute(x, (7, 5), attribute_to_neuron_input=True, **kw)
        with pytest.raises(TypeError):
            cls(object(), 4).attribute(x, (7, 5), **kw)
        with pytest.raises(AssertionError):                               # valid arguments go on to the engine
            cls(m, 4, device_ids=None).attribute(x, (-1, -1), **kw)
        with pytest.raises(TypeError):                                    # NoiseTunnel keeps refusing them
            NoiseTunnel(cls(m, 4))
    for cls in (NeuronIntegratedGradients, NeuronConductance):
        with pytest.raises(NotImplementedError):                          # a single output
            cls(m, 4).attribute(x, (7, 5), target=0)
        for kw in (dict(baselines=torch.zeros(3, 100)), dict(baselines=torch.zeros(2, 100, dtype=torch.int64)), dict(baselines="zero"),
                   dict(n_steps=0), dict(n_steps=2.5), dict(method="simpson"), dict(internal_batch_size=0),
                   dict(n_steps=1, method="riemann_left")):
            with pytest.raises(ValueError):
                cls(m, 4).attribute(x, (7, 5), **kw)
        with pytest.raises(AssertionError):
            cls(m, 4, multiply_by_inputs=False).attribute(x, (7, 5), baselines=0.05, n_steps=4, method="riemann_middle", internal_batch_size=2)
    with pytest.raises(AssertionError):
        NeuronIntegratedGradients(m, 4).attribute(x, BAND)
    for sel in (BAND, (slice(7, 8), 5), (7, slice(5, 6))):                # a slice, even of one unit
        with pytest.raises(ValueError):
            NeuronConductance(m, 4).attribute(x, sel)
    for kw in (dict(perturbations_per_eval=0), dict(feature_mask=torch.zeros(1, 100)), dict(feature_mask=torch.zeros(3, 100, dtype=torch.int64)),
               dict(baselines=torch.zeros(2, 99))):
        with pytest.raises(ValueError):
            NeuronFeatureAblation(m, 4).attribute(x, (7, 5), **kw)
    with pytest.raises(AssertionError):
        NeuronFeatureAblation(m, 4).attribute(x, BAND, feature_mask=torch.arange(100)[None] // 10, perturbations_per_eval=3)


def test_engine_validates_before_gpu_work():
    class Stub(AT.HipAttribution):
        def __init__(self):
            class E:
                nl = 9
                cfg = type("Cfg", (), {"hidden_size": H})()

                @staticmethod
                def _lengths(L):
                    return [T]
            self.eg = type("G", (), {"emb": E()})()

        def _prep(self, waves):
            raise AssertionError("the engine reached the device before rejecting its arguments")

    eng = Stub()
    x = torch.zeros(2, 100)
    shap = lambda fn: {"baselines": torch.zeros(3, 100)} if fn == eng.neuron_gradient_shap else {}
    fns = (eng.neuron_gradient, eng.neuron_integrated_gradients, eng.neuron_gradient_shap, eng.neuron_conductance,
           eng.neuron_feature_ablation)
    for fn in fns:
        kw = shap(fn)
        for bad in (-1, 10, 1.5, None):
            with pytest.raises(ValueError):
                fn(x, bad, (7, 5), **kw)
        for bad in (5, (49, 0), (0, 64), (slice(0, 4, -1), 1), (slice(9, 3), 1)):
            with pytest.raises(ValueError):
                fn(x, 4, bad, **kw)
        with pytest.raises(NotImplementedError):
            fn(x, 4, lambda h: h, **kw)
        with pytest.raises(AssertionError):
            fn(x, 4, (7, 5), **kw)
    for fn in (eng.neuron_integrated_gradients, eng.neuron_conductance):
        for kw in (dict(baselines=torch.zeros(2, 99)), dict(n_steps=0), dict(method="x"), dict(internal_batch_size=-1)):
            with pytest.raises(ValueError):
                fn(x, 4, (7, 5), **kw)
    with pytest.raises(ValueError):
        eng.neuron_conductance(x, 4, BAND)
    for kw in (dict(baselines=torch.zeros(3, 99)), dict(n_samples=0), dict(stdevs=-1.0), dict(baselines=torch.zeros(3, 100), seed=-1),
               dict(baselines=torch.zeros(3, 100), internal_batch_size=0)):
        with pytest.raises(ValueError):
            eng.neuron_gradient_shap(x, 4, (7, 5), **{**shap(eng.neuron_gradient_shap), **kw})
    for kw in (dict(feature_mask=torch.zeros(1, 100)), dict(internal_batch_size=0), dict(baselines="zero")):
        with pytest.raises(ValueError):
            eng.neuron_feature_ablation(x, 4, (7, 5), **kw)
    for bad in (0, -64.0, 48.0, float("inf"), float("nan"), "64", True):
        with pytest.raises(ValueError):
            AT.HipAttribution(None, neuron_loss_scale=bad)
    assert AT.NEURON_LOSS_SCALE > 0 and np.log2(AT.NEURON_LOSS_SCALE) % 1 == 0


def test_explainer_knows_the_neuron_methods():
    import captum_saliency as cs

    class Att:
        class eg:
            class emb:
                nl = 9
    for method in ("neuron_gradient", "neuron_integrated_gradients"):
        assert callable(cs._explainer(Att(), method, layer=4, neuron=(7, 5))) and callable(cs._explainer(Att(), method, neuron=BAND))
        with pytest.raises(ValueError):
            cs._explainer(Att(), method, layer=4)                         # no neuron
        with pytest.raises(ValueError):
            cs._explainer(Att(), method, neuron=(7, 5), nt_type="smoothgrad")


def test_argument_errors_of_the_neuron_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    fb = (C.c_float * 256)()
    p = C.addressof(fb)
    box = lambda *v: (C.c_int * 6)(*v)
    good = box(0, 2, 1, 0, 4, 1)
    bad_boxes = [box(0, 0, 1, 0, 4, 1), box(2, 1, 1, 0, 4, 1), box(0, 3, 1, 0, 4, 1), box(-1, 2, 1, 0, 4, 1), box(0, 2, 0, 0, 4, 1),
                 box(0, 2, -1, 0, 4, 1), box(0, 2, 1, 0, 0, 1), box(0, 2, 1, 0, 9, 1), box(0, 2, 1, -1, 4, 1), box(0, 2, 1, 0, 4, 0), None]
    seed = lambda src=None, rs=p, scale=1.0, R=2, T=2, H=8, b=good, resid=p, op=p, split=1, lo=32: \
        lib.advh_layer_seed(src, rs, scale, R, T, H, b, resid, op, split, lo, None)
    for bad in ([dict(resid=None), dict(R=0), dict(R=-2), dict(T=0), dict(T=-2), dict(H=0), dict(H=-8), dict(scale=float("inf")),
                 dict(scale=float("nan")), dict(lo=0), dict(lo=-32), dict(lo=31), dict(split=2), dict(split=-1),
                 dict(src=p, rs=p)] + [dict(b=b) for b in bad_boxes]):
        assert seed(**bad) == EINVAL, bad
    assert seed(src=p, rs=None, resid=None) == EINVAL and seed(src=p, rs=None, lo=31) == EINVAL      # dense mode: same contract
    vals = lambda v=p, R=2, T=2, H=8, b=good, out=p: lib.advh_neuron_values(v, R, T, H, b, out, None)
    for bad in [dict(v=None), dict(out=None), dict(R=0), dict(R=-1), dict(T=0), dict(H=0), dict(H=-8)] + [dict(b=b) for b in bad_boxes]:
        assert vals(**bad) == EINVAL, bad


def test_neuron_kernels_do_not_spill():
    res = resources("attribution_neuron.hip")
    for nm in ("layer_seed_kernel", "neuron_values_kernel"):
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == 2, (nm, sorted(res))                           # the float4 and the scalar instance
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)


def test_restated_gradient_fp32_against_fp64(model):
    """The restatement's own error: the fp32 autograd gradient against the same graph in fp64, relative to the largest entry --
    it must sit well under the 1e-4 the GPU tests allow the fp32-class chain."""
    x = syn.make_clips(2, 16000, seed=12)
    for l, sel in ((0, (7, 5)), (4, (-1, -1)), (9, BAND)):
        g32 = NR.neuron_gradient(x, l, sel, model)
        g64 = NR.neuron_gradient(x, l, sel, model, dtype=torch.float64)
        err = ((g32.double() - g64).abs().max() / g64.abs().max()).item()
        print(f"restated neuron gradient l={l} {sel}: fp32 vs fp64 {err:.3e} of max, max |g| {g64.abs().max().item():.3e}")
        assert tuple(g32.shape) == (2, 16000) and g32.dtype == torch.float32 and err < 1e-5


def test_restated_selection_is_linear(model):
    """A 2 x 2 box is the sum of its four units: the restatement's gradient of the box against the sum of the units' gradients
    (fp32 sums in another order: 1e-5 of max, ten times the fp32-versus-fp64 figure above)."""
    x = syn.make_clips(2, 16000, seed=12)
    box = NR.neuron_gradient(x, 4, (slice(7, 9), slice(5, 7)), model)
    units = sum(NR.neuron_gradient(x, 4, (t, h), model) for t in (7, 8) for h in (5, 6))
    assert ((box - units).abs().max() / box.abs().max()).item() < 1e-5


def test_restated_neuron_ig_quadrature(model):
    """NeuronIntegratedGradients of the restatement against ``s_n(x) - s_n(b)``: the delta is the rule's quadrature error
    (pre-LN: up to 1.5e-2 at 50 steps for the band), so the GPU tests compare against this delta, never against an absolute
    bound.  Here: printed, and the 50-step Gauss-Legendre delta is no larger than the 4-step one (the integrand is smooth)."""
    x = syn.make_clips(2, 16000, seed=12)
    nb = noise_baseline(2, 16000)
    for sel in ((7, 5), BAND):
        _, d50 = NR.neuron_integrated_gradients(x, nb, 4, sel, model, 50)
        _, d4 = NR.neuron_integrated_gradients(x, nb, 4, sel, model, 4)
        ds = (NR.neuron_value(x, 4, sel, model) - NR.neuron_value(nb, 4, sel, model)).tolist()
        print(f"restated NeuronIG l=4 {sel}: s_n(x) - s_n(b) {ds}, delta at 50 steps {d50.tolist()}, at 4 steps {d4.tolist()}")
        assert d50.abs().max().item() <= d4.abs().max().item()
