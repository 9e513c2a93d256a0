"""CPU-only: the layer attributions' restatement (tests/layer_attr_ref.py) is consistent with the oracle, every argument check
of the captum.attr layer classes and of the engine runs before any GPU work, the three entry points of
csrc/attribution_layer.hip keep the header's error contract and compile without scratch, and ``frames_to_wave``'s index map."""
import ctypes as C

import numpy as np
import pytest
import torch

import layer_attr_ref as LR
from addvisor_hip import _lib, attribution as AT, synthetic as syn
from oracle import wav2vec2_ref as W
from test_build_resources import resources

torch.set_grad_enabled(False)


def noise_baseline(B, L, seed=3):
    return 0.05 * torch.randn(B, L, generator=torch.Generator().manual_seed(seed))


def model_of(cfg):
    return (syn.embedder_weights(cfg), cfg) + tuple(syn.logreg_weights(cfg.hidden_size))


@pytest.fixture(scope="module", params=[False, True], ids=["post_ln", "pre_ln"])
def model(request):
    return model_of(syn.tiny_config(request.param))


def test_tail_of_a_hidden_state_is_the_classifier(model):
    x = syn.make_clips(2, 16000, seed=12)
    hs = LR.hidden(x, model)
    ref = W.classify(x, *model)[0]
    assert len(hs) == 10 and tuple(hs[0].shape) == (2, 49, 64)
    for l in (0, 4, 9):
        d = (LR.tail(hs[l], l, model) - ref).abs().max().item()
        print(f"tail(hidden_states[{l}]) vs classify: {d:.3e}")
        assert d < 1e-6


def test_tail_with_the_final_layer_norm():
    """A full-depth pre-LN encoder: ``hidden_states[nl]`` is the final LayerNorm's output, which a chain started below ``nl``
    applies and a chain started at ``nl`` does not repeat."""
    m = model_of(syn.tiny_config(True, layer_index=10))
    x = syn.make_clips(2, 16000, seed=12)
    hs = LR.hidden(x, m)
    ref = W.classify(x, *m)[0]
    for l in (0, 9, 10):
        assert (LR.tail(hs[l], l, m) - ref).abs().max().item() < 1e-6, l


def test_restated_layer_ig_is_complete(model):
    x = syn.make_clips(2, 16000, seed=12)
    for l in (0, 4, 9):
        attr, delta = LR.layer_integrated_gradients(x, noise_baseline(2, 16000), l, model, 50)
        print(f"restated LayerIG, 50 Gauss-Legendre steps, layer {l}: delta {delta.tolist()}")
        assert tuple(attr.shape) == (2, 49, 64) and delta.abs().max().item() < 1e-5


def test_restated_gradient_at_the_last_layer_is_the_pooled_coefficient(model):
    x = syn.make_clips(2, 16000, seed=12)
    g = LR.layer_gradient_x_activation(x, 9, model, multiply_by_inputs=False)
    coef = torch.as_tensor(model[2], dtype=torch.float32).view(1, 1, -1)
    assert torch.allclose(g, (coef / 49).expand_as(g), rtol=1e-6, atol=0)


def test_frame_index_map():
    for L, T, hop in ((16000, 49, 320), (16001, 49, 320), (400, 1, 320), (64000, 199, 320), (1000, 3, 7)):
        ours = AT.frame_index(L, T, hop)
        ref = np.minimum(np.arange(L) // hop, T - 1)
        assert ours.dtype == np.int64 and np.array_equal(ours, ref) and np.array_equal(ours, LR.frame_index(L, T, hop))
    assert AT.frame_index(16000, 49)[[0, 319, 320, 15679, 15680, 15999]].tolist() == [0, 0, 1, 48, 48, 48]
    with pytest.raises(ValueError):
        AT.frame_index(0, 49)


def test_check_layer():
    for l in (0, 4, 9, np.int64(3)):
        assert AT.check_layer(l, 9) == int(l)
    for bad in (-1, 10, 4.0, "4", None, True, [4], torch.tensor(4)):
        with pytest.raises(ValueError):
            AT.check_layer(bad, 9)


def test_check_layer_path_args():
    ok = dict(layer=4, nl=9, baselines=None, B=2, L=100, n_steps=4, method="gausslegendre")
    l, base, alphas, steps = AT.check_layer_path_args(**ok)
    assert l == 4 and tuple(base.shape) == (1, 100) and len(alphas) == len(steps) == 4
    assert len(AT.check_layer_path_args(**ok, extra_point=True)[2]) == 5
    assert len(AT.check_layer_path_args(**{**ok, "n_steps": 1, "method": "riemann_left"}, extra_point=True)[2]) == 2
    for bad in (dict(layer=10), dict(layer=1.5), dict(baselines=torch.zeros(3, 100)), dict(baselines=torch.zeros(2, 99)),
                dict(baselines=torch.zeros(2, 100, dtype=torch.int64)), dict(baselines="zero"), dict(n_steps=0), dict(n_steps=2.5),
                dict(n_steps=True), dict(n_steps=1, method="riemann_left"), dict(method="simpson"), dict(internal_batch_size=0),
                dict(internal_batch_size=1.5)):
        with pytest.raises(ValueError):
            AT.check_layer_path_args(**{**ok, **bad})


class _NoEngine:
    def num_layers(self):
        return 9

    def hip_attribution(self):
        raise AssertionError("the front end reached the engine before rejecting its arguments")


def test_front_end_validates_before_gpu_work():
    from captum.attr import (InternalInfluence, LayerActivation, LayerConductance, LayerGradientXActivation, LayerIntegratedGradients,
                             NoiseTunnel)
    import captum_saliency
    for name in ("LayerActivation", "LayerGradientXActivation", "LayerIntegratedGradients", "LayerConductance", "InternalInfluence"):
        assert getattr(captum_saliency, name) is getattr(__import__("captum.attr", fromlist=[name]), name)
    x = torch.zeros(2, 100)
    m = _NoEngine()
    classes = (LayerActivation, LayerGradientXActivation, LayerIntegratedGradients, LayerConductance, InternalInfluence)
    path = (LayerIntegratedGradients, LayerConductance, InternalInfluence)
    for cls in classes:
        for bad in (-1, 10, 2.0, "4", None, True):                       # a layer out of range or not an int
            with pytest.raises(ValueError):
                cls(m, bad).attribute(x)
        with pytest.raises(ValueError):
            cls(m, 4).attribute(x[0])
        with pytest.raises(NotImplementedError):
            cls(m, 4).attribute(x, attribute_to_layer_input=True)
        with pytest.raises(TypeError):
            cls(object(), 4).attribute(x)
        with pytest.raises(AssertionError):                               # valid arguments go on to the engine
            cls(m, 4).attribute(x)
        with pytest.raises(TypeError):                                    # layer maps are [B, T, H]: NoiseTunnel does not wrap them
            NoiseTunnel(cls(m, 4))
    for cls in classes[1:]:
        with pytest.raises(NotImplementedError):                          # a single output
            cls(m, 4).attribute(x, target=0)
    for cls in path:
        for kw in (dict(baselines=torch.zeros(3, 100)), dict(baselines=torch.zeros(2, 100, dtype=torch.int64)), dict(baselines="zero"),
                   dict(n_steps=0), dict(n_steps=2.5), dict(method="simpson"), dict(internal_batch_size=0)):
            with pytest.raises(ValueError):
                cls(m, 4).attribute(x, **kw)
        with pytest.raises(AssertionError):
            cls(m, 4).attribute(x, baselines=0.05, n_steps=4, method="riemann_middle", internal_batch_size=2)
    for cls in (LayerIntegratedGradients, InternalInfluence):             # a Riemann rule needs two points: n_steps = 1 is one ...
        with pytest.raises(ValueError):
            cls(m, 4).attribute(x, n_steps=1, method="riemann_left")
    with pytest.raises(AssertionError):                                   # ... and two for LayerConductance
        LayerConductance(m, 4).attribute(x, n_steps=1, method="riemann_left")
    with pytest.raises(NotImplementedError):
        LayerConductance(m, 4).attribute(x, return_convergence_delta=True)


def test_engine_validates_before_gpu_work():
    class Stub(AT.HipAttribution):
        def __init__(self):
            class E:
                nl = 9
            self.eg = type("G", (), {"emb": E()})()

        def _prep(self, waves):
            raise AssertionError("the engine reached the device before rejecting its arguments")

    eng = Stub()
    x = torch.zeros(2, 100)
    for fn in (eng.layer_activation, eng.layer_gradient_x_activation, eng.layer_integrated_gradients, eng.layer_conductance,
               eng.internal_influence):
        for bad in (-1, 10, 1.5, None):
            with pytest.raises(ValueError):
                fn(x, bad)
        with pytest.raises(AssertionError):
            fn(x, 4)
    for fn in (eng.layer_integrated_gradients, eng.layer_conductance, eng.internal_influence):
        for kw in (dict(baselines=torch.zeros(2, 99)), dict(n_steps=0), dict(method="x"), dict(internal_batch_size=-1)):
            with pytest.raises(ValueError):
                fn(x, 4, **kw)
    with pytest.raises(NotImplementedError):
        eng.layer_integrated_gradients(x, 4, multiply_by_inputs=False, return_convergence_delta=True)


def test_explainer_knows_the_layer_methods():
    import captum_saliency as cs

    class Att:
        class eg:
            class emb:
                nl = 9
    for method in ("layer_integrated_gradients", "layer_gradient_x_activation"):
        assert callable(cs._explainer(Att(), method, layer=4)) and callable(cs._explainer(Att(), method))
        with pytest.raises(ValueError):
            cs._explainer(Att(), method, nt_type="smoothgrad")


def test_argument_errors_of_the_layer_entry_points():
    """include/addvisor_hip.h error contract (negative return, nothing launched): validation happens before any HIP call, so it
    runs without a GPU."""
    lib = _lib.lib()
    EINVAL = -1
    fb = (C.c_float * 256)()
    p = C.addressof(fb)
    inject = lambda src=p, rows=4, n=16, resid=p, op=p, split=1, lo=64: lib.advh_layer_inject(src, rows, n, resid, op, split, lo, None)
    for bad in (dict(src=None), dict(resid=None), dict(rows=0), dict(rows=-4), dict(n=0), dict(n=-16), dict(lo=0), dict(lo=-64),
                dict(lo=63), dict(split=2), dict(split=-1)):
        assert inject(**bad) == EINVAL, bad
    tap = lambda g=p, act=p, s=1.0, rows=4, n=16, out=p, rs=p: lib.advh_layer_tap(g, act, s, rows, n, out, rs, None)
    for bad in (dict(g=None), dict(out=None, rs=None), dict(rows=0), dict(rows=-1), dict(n=0), dict(n=-16), dict(s=float("inf")),
                dict(s=float("nan"))):
        assert tap(**bad) == EINVAL, bad
    cond = lambda grad=p, act=p, B=2, n=16, steps=3, ngrad=3, first=1, pg=p, pa=p, tot=p: \
        lib.advh_layer_conductance_accumulate(grad, act, B, n, steps, ngrad, first, pg, pa, tot, None)
    for bad in (dict(grad=None), dict(act=None), dict(pg=None), dict(pa=None), dict(tot=None), dict(B=0), dict(B=-2), dict(n=0),
                dict(n=-1), dict(steps=0), dict(steps=-3), dict(ngrad=-1), dict(ngrad=4), dict(first=2), dict(first=-1)):
        assert cond(**bad) == EINVAL, bad


def test_layer_kernels_do_not_spill():
    res = resources("attribution_layer.hip")
    for nm in ("layer_inject_kernel", "layer_tap_kernel", "layer_tap_row_sum_kernel", "layer_conductance_kernel"):
        hit = {k: v for k, v in res.items() if nm in k}
        assert len(hit) == 2, (nm, sorted(res))                           # the float4 and the scalar instance
        for k, v in hit.items():
            assert v["scratch"] == 0, (k, v)
