"""CPU restatement of Captum's Occlusion and FeatureAblation for tests/test_ablation_cpu.py and tests/test_gpu_ablation.py,
written the way Captum computes them (captum is absent; restated from ``captum.attr._core.occlusion`` /
``feature_ablation``): one 0/1 mask per perturbation (Occlusion: ``ones(win)`` padded by ``k * stride`` on the left and by
``L - k * stride - win`` on the right, a negative right pad cropping the last window; FeatureAblation: ``mask == id`` for every
id in ``[min, max]``, as Captum up to 0.7 loops), ablated inputs ``x * (1 - m) + base * m`` repeated perturbation-major, and
``total += diff * m; weights += m; total / weights`` (Occlusion) or ``total`` (FeatureAblation).

The forward is pluggable: a callable ``[rows, L] -> [rows]`` logits (``model_forward`` wraps
``oracle.attribution_ref.model_logit``), or given logits ``f0 [B]`` and ``fk [K * B]`` (row ``k * B + b``)."""
import math

import torch
import torch.nn.functional as F

from oracle import attribution_ref as A


def model_forward(model, rows_per_call=16):
    """``oracle.attribution_ref.model_logit`` (fp32, CPU) as ``[rows, L] -> [rows]``, ``rows_per_call`` rows at a time."""
    def fwd(w):
        with torch.no_grad():
            return torch.cat([A.model_logit(w[i:i + rows_per_call], *model).view(-1) for i in range(0, w.shape[0], rows_per_call)])
    return fwd


def occlusion_masks(L, win, stride):
    """``[K, 1, L]`` float masks, Captum's ``_occlusion_mask`` for a 1-D input."""
    K = math.ceil((L - win) / stride) + 1
    ones = torch.ones(win)
    return torch.stack([F.pad(ones, (k * stride, L - (k * stride + win))) for k in range(K)])[:, None]


def feature_masks(feature_mask, L):
    """``[K, 1 | B, L]`` float masks, one per id in ``[min, max]`` of ``feature_mask`` (None: every sample its own feature)."""
    if feature_mask is None:
        feature_mask = torch.arange(L)[None]
    lo, hi = int(feature_mask.min()), int(feature_mask.max())
    return torch.stack([(feature_mask == j) for j in range(lo, hi + 1)]).to(torch.float32)


def ablated_batch(x, base, masks):
    """``[K * B, L]``: row ``k * B + b`` = ``x[b] * (1 - m_k) + base * m_k`` (Captum's ``input.repeat`` order)."""
    B, L = x.shape
    K = masks.shape[0]
    m = masks.expand(K, B, L).reshape(K * B, L)
    return x.repeat(K, 1) * (1 - m) + base.expand(B, L).repeat(K, 1) * m


def _baseline(base, B, L):
    return torch.full((1, L), float(base)) if isinstance(base, (int, float)) else base.to(torch.float32)


def _attribute(x, base, masks, use_weights, forward=None, f0=None, fk=None):
    B, L = x.shape
    K = masks.shape[0]
    base = _baseline(base, B, L)
    if forward is not None:
        f0 = forward(x).view(-1)
        fk = forward(ablated_batch(x, base, masks)).view(-1)
    fk = fk.view(K, B)
    total = torch.zeros(B, L)
    weights = torch.zeros(B, L)
    for k in range(K):
        m = masks[k].expand(B, L)
        diff = f0 - fk[k]
        total += diff[:, None] * m
        weights += m
    return total / weights if use_weights else total


def occlusion(x, base, win, stride, forward=None, f0=None, fk=None):
    """Captum's Occlusion of ``x [B, L]``: ``(attr [B, L], K)``."""
    masks = occlusion_masks(x.shape[1], win, stride)
    return _attribute(x, base, masks, True, forward, f0, fk), masks.shape[0]


def feature_ablation(x, base, feature_mask, forward=None, f0=None, fk=None):
    """Captum's FeatureAblation of ``x [B, L]`` (ids ``[min, max]``): ``(attr [B, L], K)``."""
    masks = feature_masks(feature_mask, x.shape[1])
    return _attribute(x, base, masks, False, forward, f0, fk), masks.shape[0]
