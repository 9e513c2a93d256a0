"""CPU restatement of the neuron attributions (Captum 0.7's NeuronGradient, NeuronIntegratedGradients, NeuronGradientShap,
NeuronConductance, NeuronFeatureAblation of ``hidden_states[l]`` of the encoder), for tests/test_neuron_attr_cpu.py and
tests/test_gpu_neuron_attr.py.  fp32 autograd through ``oracle.wav2vec2_ref.hidden_states(zero_mean_unit_var_norm(x), ...)[l]``;
the quadrature tables and the ablation loop are those of tests/attribution_baselines_ref.py and tests/ablation_ref.py.
Parity with Captum is unpinned (captum is absent): the formulas are restated.

``model`` is ``(sd, cfg, coef, intercept)`` as in tests/attribution_baselines_ref.py.  A selector is a ``(t, h)`` tuple of ints or
slices; ``s_n(x)[b]`` is the sum of ``hidden_states[l](x)[b][selector]`` (Captum aggregates slices by sum)."""
import torch

import ablation_ref as AB
import layer_attr_ref as LR
from attribution_baselines_ref import approximation
from oracle import wav2vec2_ref as W
from oracle.signal_ref import zero_mean_unit_var_norm


def select(h, selector):
    """``h [R, T, H] -> [R]``: the sum over the selection (plain Python indexing, one axis at a time)."""
    t, c = selector
    v = h[:, t] if isinstance(t, slice) else h[:, [t]]
    v = v[:, :, c] if isinstance(c, slice) else v[:, :, [c]]
    return v.reshape(h.shape[0], -1).sum(1)


def neuron_value(x, l, selector, model, dtype=torch.float32):
    """``s_n(x) [R]`` (differentiable)."""
    sd, cfg, _, _ = model
    if dtype != torch.float32:
        sd = {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}
    return select(W.hidden_states(zero_mean_unit_var_norm(x.to(dtype)), sd, cfg, upto=cfg.layer_index)[l], selector)


def neuron_gradient(x, l, selector, model, dtype=torch.float32, rows_per_call=8):
    """``d s_n / d x [R, L]``."""
    out = []
    for i in range(0, x.shape[0], rows_per_call):
        with torch.enable_grad():
            xi = x[i:i + rows_per_call].to(dtype).clone().detach().requires_grad_(True)
            (g,) = torch.autograd.grad(neuron_value(xi, l, selector, model, dtype).sum(), xi)
        out.append(g)
    return torch.cat(out)


def _path(x, base, method, n):
    B, L = x.shape
    b = base.expand(B, L).to(x.dtype)
    alphas, steps = approximation(method, n)
    return b, [b + float(a) * (x - b) for a in alphas], steps


def neuron_integrated_gradients(x, base, l, selector, model, n_steps=50, method="gausslegendre", multiply_by_inputs=True):
    """``integrated_gradients`` with ``s_n`` in the place of the logit.  Returns ``(attr [B, L], delta [B] float64)``,
    ``delta = sum attr - (s_n(x) - s_n(b))`` (Captum's class returns no delta; the tests use it as the quadrature error)."""
    B, L = x.shape
    b, pts, steps = _path(x, base, method, n_steps)
    g = neuron_gradient(torch.cat(pts), l, selector, model).view(n_steps, B, L)             # step-major rows
    total = (g * torch.tensor(steps, dtype=x.dtype)[:, None, None]).sum(0)
    attr = total * (x - b) if multiply_by_inputs else total
    with torch.no_grad():
        ds = neuron_value(x, l, selector, model).double() - neuron_value(b, l, selector, model).double()
    return attr, attr.double().sum(1) - ds


def neuron_gradient_shap(x, base, idx, alpha, noise, sigma, S, l, selector, model, multiply_by_inputs=True):
    """``gradient_shap`` of tests/attribution_baselines_ref.py with ``s_n``, fed explicit draws (expanded rows ``b * S + s``)."""
    B, L = x.shape
    xt = x.repeat_interleave(S, 0) + sigma * noise.to(x.dtype)
    bt = base.to(x.dtype)[torch.as_tensor(idx).long()]
    a = torch.as_tensor(alpha, dtype=x.dtype)[:, None]
    g = neuron_gradient(bt + a * (xt - bt), l, selector, model)
    return ((xt - bt) * g if multiply_by_inputs else g).view(B, S, L).sum(1) / S


def neuron_conductance(x, base, l, neuron, model, n_steps=50, method="gausslegendre", multiply_by_inputs=True):
    """A single neuron ``h_n`` (two ints): ``(x - b) * sum_k w_k dF/dh_n(x_k) * (d h_n / d x)(x_k)`` over the ``n_steps``
    waveform-space points of the rule."""
    B, L = x.shape
    b, pts, steps = _path(x, base, method, n_steps)
    rows = torch.cat(pts)
    m = select(LR.layer_gradient(LR.hidden(rows, model)[l], l, model), neuron)               # dF/dh_n of every point
    g = (m[:, None] * neuron_gradient(rows, l, neuron, model)).view(n_steps, B, L)
    total = (g * torch.tensor(steps, dtype=x.dtype)[:, None, None]).sum(0)
    return total * (x - b) if multiply_by_inputs else total


def neuron_forward(l, selector, model, rows_per_call=16):
    """``s_n`` as the pluggable forward ``[rows, L] -> [rows]`` of tests/ablation_ref.py."""
    def fwd(w):
        with torch.no_grad():
            return torch.cat([neuron_value(w[i:i + rows_per_call], l, selector, model) for i in range(0, w.shape[0], rows_per_call)])
    return fwd


def neuron_feature_ablation(x, base, feature_mask, l, selector, model):
    """``feature_ablation`` of tests/ablation_ref.py with ``s_n`` in the place of the logit: ``attr [B, L]``."""
    return AB.feature_ablation(x, base, feature_mask, neuron_forward(l, selector, model))[0]
