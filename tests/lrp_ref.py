"""CPU restatement of conservative propagation through the transformer encoder (Ali et al., ICML 2022, "XAI for Transformers:
Better Explanations through Conservative Propagation": the LN-rule and the AH-rule; the GELU identity rule of AttnLRP, Achtibat et
al. 2024), for tests/test_lrp_cpu.py and tests/test_gpu_lrp.py.  Captum has no rule for LayerNorm, softmax attention or GELU and
the reference has no such method: the formulas are restated from the publications, parity is unpinned.

The method is gradient x input through a copy of the encoder with ``.detach()`` at three places: a LayerNorm written out with a
detached ``1/sigma``, the attention of tests/attention_rollout_ref.py with detached probabilities, and the oracle's
``feed_forward`` body with ``GELU(x) = x * Phi(x).detach()``.  Evaluated in float64 by default, so that the engine's fp32-class bar
never measures the yardstick's own rounding.

``model`` is ``(sd, cfg, coef, intercept)`` as in tests/attention_rollout_ref.py."""
import math

import torch
import torch.nn.functional as F

import attention_rollout_ref as AR
from oracle import wav2vec2_ref as W
from oracle.signal_ref import zero_mean_unit_var_norm

GELU_RULES = ("gradient", "identity")


def layer_norm(t, weight, bias, eps, frozen):
    """``F.layer_norm`` over the last axis written out; ``frozen``: ``1/sigma`` is a constant of the backward pass (the centring
    stays differentiable)."""
    c = t - t.mean(-1, keepdim=True)
    rstd = (c.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return c * (rstd.detach() if frozen else rstd) * weight + bias


def attention(h, sd, p, nheads, frozen):
    """attention_rollout_ref._attention; ``frozen``: the probabilities are a constant of the backward pass."""
    B, T, H = h.shape
    d = H // nheads
    q = F.linear(h, sd[p + "q_proj.weight"], sd[p + "q_proj.bias"]).view(B, T, nheads, d).transpose(1, 2)
    k = F.linear(h, sd[p + "k_proj.weight"], sd[p + "k_proj.bias"]).view(B, T, nheads, d).transpose(1, 2)
    v = F.linear(h, sd[p + "v_proj.weight"], sd[p + "v_proj.bias"]).view(B, T, nheads, d).transpose(1, 2)
    a = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * d ** -0.5, dim=-1)
    ctx = torch.matmul(a.detach() if frozen else a, v)
    return F.linear(ctx.transpose(1, 2).reshape(B, T, H), sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def feed_forward(h, sd, p, gelu_rule):
    """oracle.wav2vec2_ref.feed_forward; ``"identity"``: ``GELU(x) = x * Phi(x).detach()``."""
    z = F.linear(h, sd[p + "intermediate_dense.weight"], sd[p + "intermediate_dense.bias"])
    if gelu_rule == "identity":
        z = z * (0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))).detach()
    else:
        z = F.gelu(z)
    return F.linear(z, sd[p + "output_dense.weight"], sd[p + "output_dense.bias"])


def zero_bias_model(model):
    """The model with every bias and LayerNorm beta of the encoder layers and of ``encoder.layer_norm``, and the logreg's
    intercept, set to zero: with all three rules on, ``hidden_states[start_layer] -> F~`` is linear and relevance is conserved."""
    sd, cfg, coef, icpt = model
    sd = {k: (torch.zeros_like(v) if (k.startswith("encoder.layer") and k.endswith(".bias")) else v) for k, v in sd.items()}
    return sd, cfg, coef, icpt * 0


def explain(x, model, target=None, start_layer=0, ln_rule=True, attention_rule=True, gelu_rule="gradient", dtype=torch.float64):
    """``logits [B]`` (of the unmodified classifier: the rules change no forward value), ``x = hidden_states[start_layer]``,
    ``grad = d(+-F~)/dx``, ``R = x * grad`` ``[B, T, H]`` and ``rel = sum_h R`` ``[B, T]``, in ``dtype``."""
    assert gelu_rule in GELU_RULES
    sd, cfg, coef, icpt = model
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    eps, nl, heads = cfg.layer_norm_eps, AR.num_layers(cfg), cfg.num_attention_heads
    assert 0 <= start_layer < nl

    def layer(h, l, ln_f, att_f, gelu):
        p = f"encoder.layers.{l}."
        ln = lambda t, q: layer_norm(t, sd[p + q + ".weight"], sd[p + q + ".bias"], eps, ln_f)
        if cfg.do_stable_layer_norm:
            h = h + attention(ln(h, "layer_norm"), sd, p + "attention.", heads, att_f)
            return h + feed_forward(ln(h, "final_layer_norm"), sd, p + "feed_forward.", gelu)
        h = ln(h + attention(h, sd, p + "attention.", heads, att_f), "layer_norm")
        return ln(h + feed_forward(h, sd, p + "feed_forward.", gelu), "final_layer_norm")

    with torch.no_grad():
        h = W.hidden_states(zero_mean_unit_var_norm(x.to(dtype)), sd, cfg, upto=0)[0]
        for l in range(start_layer):
            h = layer(h, l, False, False, "gradient")
    with torch.enable_grad():
        x0 = h.clone().requires_grad_(True)
        h = x0
        for l in range(start_layer, nl):
            h = layer(h, l, ln_rule, attention_rule, gelu_rule)
        if cfg.do_stable_layer_norm and nl == cfg.num_hidden_layers:
            h = layer_norm(h, sd["encoder.layer_norm.weight"], sd["encoder.layer_norm.bias"], eps, ln_rule)
        logits = F.linear(h.mean(dim=1), torch.as_tensor(coef, dtype=dtype), torch.as_tensor(icpt, dtype=dtype)).view(-1)
        sign = AR.target_sign(target, logits)
        (grad,) = torch.autograd.grad((sign * logits).sum(), x0)
    x0 = x0.detach()
    R = x0 * grad
    return dict(logits=logits.detach(), x=x0, grad=grad, R=R, rel=R.sum(-1), sign=sign)
