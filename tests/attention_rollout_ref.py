"""CPU restatement of the attention maps, attention rollout (Abnar & Zuidema 2020) and gradient-weighted rollout (the
self-attention rule of Chefer et al. 2021) of the encoder, for tests/test_attention_rollout_cpu.py and
tests/test_gpu_attention_rollout.py.  Captum has no class for these methods and neither has the reference: the formulas are
restated from the publications, parity is unpinned.

The encoder is restated from the oracle's ``feed_forward`` and ``hidden_states(..., upto=0)`` with an attention that keeps its
probabilities ``a`` (``retain_grad``), and the oracle's logreg formula in the working dtype; it is evaluated in float64 by
default (weights and clips cast to double), so that the engine's fp32-class bar never measures the yardstick's own rounding.

``model`` is ``(sd, cfg, coef, intercept)`` as in tests/layer_attr_ref.py."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import wav2vec2_ref as W
from oracle.signal_ref import zero_mean_unit_var_norm

FUSIONS = ("mean", "max", "min")


def num_layers(cfg) -> int:
    return min(cfg.layer_index, cfg.num_hidden_layers)


def fuse_heads(a, fusion):
    """``[B, heads, T, T] -> [B, T, T]``."""
    return a.mean(1) if fusion == "mean" else (a.max(1).values if fusion == "max" else a.min(1).values)


def target_sign(target, logits):
    """The per-clip sign of the explained output: None / 1 -> +F, 0 -> -F, "predicted" -> sign(F(x_b)) F, a [B] tensor of 0 / 1."""
    B = logits.shape[0]
    if target is None:
        return torch.ones(B, dtype=logits.dtype)
    if isinstance(target, str):
        assert target == "predicted"
        return torch.sign(logits.detach().view(-1))
    if torch.is_tensor(target):
        return target.to(logits.dtype) * 2 - 1
    return torch.full((B,), 2.0 * int(target) - 1.0, dtype=logits.dtype)


def _attention(h, sd, p, nheads, keep):
    """oracle.wav2vec2_ref.attention, keeping the probabilities, the values and the context of every head."""
    B, T, H = h.shape
    d = H // nheads
    q = F.linear(h, sd[p + "q_proj.weight"], sd[p + "q_proj.bias"]).view(B, T, nheads, d).transpose(1, 2)
    k = F.linear(h, sd[p + "k_proj.weight"], sd[p + "k_proj.bias"]).view(B, T, nheads, d).transpose(1, 2)
    v = F.linear(h, sd[p + "v_proj.weight"], sd[p + "v_proj.bias"]).view(B, T, nheads, d).transpose(1, 2)
    a = torch.softmax(torch.matmul(q, k.transpose(2, 3)) * d ** -0.5, dim=-1)
    ctx = torch.matmul(a, v)
    if a.requires_grad:
        a.retain_grad()
        ctx.retain_grad()
    keep.append((a, v, ctx))
    return F.linear(ctx.transpose(1, 2).reshape(B, T, H), sd[p + "out_proj.weight"], sd[p + "out_proj.bias"])


def encoder(x, model, dtype=torch.float64):
    """``(logits [B], keep)``: the classifier on the clips ``x [B, L]`` in ``dtype``; ``keep[l] = (a, v, ctx)`` of layer ``l``,
    part of the autograd graph of ``logits``."""
    sd, cfg, coef, icpt = model
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    H, eps, nl = cfg.hidden_size, cfg.layer_norm_eps, num_layers(cfg)
    ln = lambda t, p: F.layer_norm(t, (H,), sd[p + ".weight"], sd[p + ".bias"], eps)
    with torch.no_grad():
        h = W.hidden_states(zero_mean_unit_var_norm(x.to(dtype)), sd, cfg, upto=0)[0]
    keep = []
    with torch.enable_grad():
        h = h.clone().requires_grad_(True)
        for l in range(nl):
            p = f"encoder.layers.{l}."
            if cfg.do_stable_layer_norm:
                h = h + _attention(ln(h, p + "layer_norm"), sd, p + "attention.", cfg.num_attention_heads, keep)
                h = h + W.feed_forward(ln(h, p + "final_layer_norm"), sd, p + "feed_forward.")
            else:
                h = ln(h + _attention(h, sd, p + "attention.", cfg.num_attention_heads, keep), p + "layer_norm")
                h = ln(h + W.feed_forward(h, sd, p + "feed_forward."), p + "final_layer_norm")
        if cfg.do_stable_layer_norm and nl == cfg.num_hidden_layers:
            h = ln(h, "encoder.layer_norm")
        # oracle.wav2vec2_ref.logreg in the working dtype
        logits = F.linear(h.mean(dim=1), torch.as_tensor(coef, dtype=dtype), torch.as_tensor(icpt, dtype=dtype)).view(-1)
    return logits, keep


def rollout(A, fusion, start_layer=0):
    """``R [B, T, T]``: ``R = I``, ``R <- rownorm(R + M R)`` over the layers ``>= start_layer``, ``M`` the fused probabilities."""
    B, _, T, _ = A[0].shape
    R = torch.eye(T, dtype=A[0].dtype).expand(B, T, T).clone()
    for a in A[start_layer:]:
        M = fuse_heads(a, fusion)
        R = (R + M @ R) / (1 + M.sum(-1, keepdim=True))
    return R


def grad_rollout(Abar, start_layer=0):
    """``D = R - I`` of ``R <- R + Abar_l R``: ``D_0 = 0``, ``D <- D + Abar_l + Abar_l D`` over the layers ``>= start_layer``."""
    D = torch.zeros_like(Abar[0])
    for ab in Abar[start_layer:]:
        D = D + ab + ab @ D
    return D


def explain(x, model, target=None, start_layer=0, dtype=torch.float64):
    """Every quantity of the three methods at the clips ``x``:
    ``logits [B]``; per layer ``A`` (probabilities), ``G = d(+-F)/dA``, ``G_ctx = dO V^T`` (the same gradient from the gradient at
    the attention context), ``GA = (G * A)^+`` ``[B, heads, T, T]`` and ``Abar = mean_h GA`` ``[B, T, T]``; ``R[fusion]`` and
    ``rel[fusion]`` of the plain rollout; ``D`` and ``rel_grad`` of the gradient rollout."""
    logits, keep = encoder(x, model, dtype)
    sign = target_sign(target, logits)
    with torch.enable_grad():
        (sign * logits).sum().backward()
    A = [a.detach() for a, _, _ in keep]
    G = [a.grad for a, _, _ in keep]
    G_ctx = [c.grad @ v.detach().transpose(2, 3) for _, v, c in keep]
    GA = [(g * a).clamp_min(0) for g, a in zip(G, A)]
    Abar = [t.mean(1) for t in GA]
    R = {f: rollout(A, f, start_layer) for f in FUSIONS}
    D = grad_rollout(Abar, start_layer)
    return dict(logits=logits.detach(), A=A, G=G, G_ctx=G_ctx, GA=GA, Abar=Abar, R=R, rel={f: r.mean(1) for f, r in R.items()},
                D=D, rel_grad=D.mean(1))


def frame_index(L, T, hop=320):
    return np.minimum(np.arange(L) // hop, T - 1)
