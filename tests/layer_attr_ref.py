"""CPU restatement of the layer attributions (Captum 0.7's LayerActivation, LayerGradientXActivation,
LayerIntegratedGradients, LayerConductance, InternalInfluence at ``hidden_states[l]`` of the encoder), for
tests/test_layer_attr_cpu.py and tests/test_gpu_layer_attr.py.  fp32 autograd on ``tail`` -- the classifier from a layer's
activation on, built from the oracle's ``attention`` / ``feed_forward`` / ``logreg`` -- and on ``oracle.wav2vec2_ref.hidden_states``.
Parity with Captum is unpinned (captum is absent): the formulas are restated.

``model`` is ``(sd, cfg, coef, intercept)`` as in tests/attribution_baselines_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from attribution_baselines_ref import approximation
from oracle import wav2vec2_ref as W
from oracle.signal_ref import zero_mean_unit_var_norm


def num_layers(cfg) -> int:
    return min(cfg.layer_index, cfg.num_hidden_layers)


def tail(h, l, model):
    """``hidden_states[l] [R, T, H] -> logits [R, 1]``: layers ``l .. nl-1``, the final LayerNorm where the model has one (a
    full-depth pre-LN encoder; it produces ``hidden_states[nl]``, so it is not applied again to a chain started at ``nl``), the
    mean over time and the logreg."""
    sd, cfg, coef, icpt = model
    H, eps, nl = cfg.hidden_size, cfg.layer_norm_eps, num_layers(cfg)
    ln = lambda t, p: F.layer_norm(t, (H,), sd[p + ".weight"], sd[p + ".bias"], eps)
    for k in range(l, nl):
        p = f"encoder.layers.{k}."
        if cfg.do_stable_layer_norm:
            h = h + W.attention(ln(h, p + "layer_norm"), sd, p + "attention.", cfg.num_attention_heads)
            h = h + W.feed_forward(ln(h, p + "final_layer_norm"), sd, p + "feed_forward.")
        else:
            h = ln(h + W.attention(h, sd, p + "attention.", cfg.num_attention_heads), p + "layer_norm")
            h = ln(h + W.feed_forward(h, sd, p + "feed_forward."), p + "final_layer_norm")
    if cfg.do_stable_layer_norm and nl == cfg.num_hidden_layers and l < nl:
        h = ln(h, "encoder.layer_norm")
    return W.logreg(h.mean(dim=1), coef, icpt)[0]


def hidden(x, model):
    """Every ``hidden_states[0 .. nl]`` of the waveforms ``x [B, L]``."""
    sd, cfg, _, _ = model
    with torch.no_grad():
        return W.hidden_states(zero_mean_unit_var_norm(x), sd, cfg, upto=cfg.layer_index)


def logit(x, model):
    with torch.no_grad():
        return W.classify(x, *model)[0].view(-1)


def layer_gradient(h, l, model):
    """``dF/dh_l`` at the activations ``h [R, T, H]``."""
    with torch.enable_grad():
        h = h.clone().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(tail(h, l, model).sum(), h)
    return g


def layer_gradient_x_activation(x, l, model, multiply_by_inputs=True):
    h = hidden(x, model)[l]
    g = layer_gradient(h, l, model)
    return g * h if multiply_by_inputs else g


def _path(x, base, method, n):
    B, L = x.shape
    b = base.expand(B, L).to(x.dtype)
    alphas, steps = approximation(method, n)
    return b, [b + float(a) * (x - b) for a in alphas], steps


def layer_integrated_gradients(x, base, l, model, n_steps=50, method="gausslegendre", multiply_by_inputs=True):
    """Path ``hb + alpha (hx - hb)`` in the layer's activation space; returns ``(attr [B, T, H], delta [B] float64)``,
    ``delta = sum attr - (F(x) - F(b))``."""
    B, L = x.shape
    b = base.expand(B, L).to(x.dtype)
    hx, hb = hidden(x, model)[l], hidden(b, model)[l]
    alphas, steps = approximation(method, n_steps)
    total = torch.zeros_like(hx)
    for a, s in zip(alphas, steps):
        total += float(s) * layer_gradient(hb + float(a) * (hx - hb), l, model)
    attr = total * (hx - hb) if multiply_by_inputs else total
    return attr, attr.double().sum((1, 2)) - (logit(x, model).double() - logit(b, model).double())


def layer_conductance(x, base, l, model, n_steps=50, method="gausslegendre"):
    """``sum_{k < n_steps} g_k (h_{k+1} - h_k)`` over the ``n_steps + 1`` waveform-space points of the rule."""
    _, pts, _ = _path(x, base, method, n_steps + 1)
    hs = [hidden(p, model)[l] for p in pts]
    total = torch.zeros_like(hs[0])
    for k in range(n_steps):
        total += layer_gradient(hs[k], l, model) * (hs[k + 1] - hs[k])
    return total


def internal_influence(x, base, l, model, n_steps=50, method="gausslegendre"):
    """``sum_k w_k g_k`` over the ``n_steps`` waveform-space points of the rule."""
    _, pts, steps = _path(x, base, method, n_steps)
    total = None
    for p, s in zip(pts, steps):
        g = float(s) * layer_gradient(hidden(p, model)[l], l, model)
        total = g if total is None else total + g
    return total


def frame_index(L, T, hop=320):
    return np.minimum(np.arange(L) // hop, T - 1)
