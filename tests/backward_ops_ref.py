"""fp64 restatement of the input-gradient chain's row / attention kernels (csrc/backward.hip, attention_bwd_x3.hip,
attention_bwd_f32.hip), for tests/test_gpu_backward_kernels.py.

Explicit formulas, not autograd, written from the mathematics -- tests/test_backward_ops_ref_cpu.py pins them against
``torch.autograd`` in float64.  Every function computes in float64 whatever dtype it is handed.
"""
import math

import torch

from embedder_ops_ref import gelu_grad


def layernorm_bwd(x, dy, gamma, beta, eps, gelu_fwd, dact_src=None, add=None):
    """dx of ``y = LN(x) * gamma + beta`` [then GELU if ``gelu_fwd``] over the last dim, given dy:
        g  = dy * [GELU'(xhat * gamma + beta)] * gamma
        dx = rstd * (g - mean(g) - xhat * mean(g * xhat))
    then ``* GELU'(dact_src)``, then ``+ add``.  Biased variance, eps inside the square root."""
    x, dy, gamma = x.double(), dy.double(), gamma.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    g = dy
    if gelu_fwd:
        g = g * gelu_grad(xhat * gamma + beta.double())
    g = g * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if dact_src is not None:
        dx = dx * gelu_grad(dact_src)
    if add is not None:
        dx = dx + add.double()
    return dx


def _r16(t, on):
    return t.to(torch.float16).double() if on else t


def attention_bwd_f16_model(q, k, v, dO, rounding=True):
    """Gradients of ``softmax(q k^T / sqrt(d)) v`` on [..., T, d] given dO, in float64, with operands rounded to fp16 exactly
    where ``attention_bwd_kernel`` (csrc/backward.hip) rounds them:
      * P = softmax(S) and delta = rowsum(P * dP) stay fp32 there (backward.hip:254-275): not rounded here;
      * dS * scale = P (dP - delta) scale is converted to fp16 before dQ = dS K (backward.hip:282-285) and before
        dK = dS^T Q (backward.hip:375, 378);
      * P is converted to fp16 before dV = P^T dO (backward.hip:373-377);
      * dQ (backward.hip:312), dK and dV (backward.hip:406-407) are stored as fp16.
    Returns a dict: dq, dk, dv (rounded), p, ds (``dS * scale`` before its rounding) and dq_pre / dk_pre / dv_pre, the
    fp64 sums in front of the output conversion.  ``rounding=False`` is the plain restatement."""
    q, k, v, dO = q.double(), k.double(), v.double(), dO.double()
    scale = 1.0 / math.sqrt(q.shape[-1])
    p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    dp = dO @ v.transpose(-1, -2)
    delta = (p * dp).sum(-1, keepdim=True)
    ds = p * (dp - delta) * scale
    ds_op, p_op = _r16(ds, rounding), _r16(p, rounding)
    pre = {"dq_pre": ds_op @ k, "dk_pre": ds_op.transpose(-1, -2) @ q, "dv_pre": p_op.transpose(-1, -2) @ dO}
    out = {n[:2]: _r16(t, rounding) for n, t in pre.items()}
    return {**out, **pre, "p": p, "ds": ds}


def attention_bwd(q, k, v, dO):
    """(dq, dk, dv, P, dS) of ``softmax(q k^T / sqrt(d)) v`` on [..., T, d]: dV = P^T dO, dP = dO V^T,
    dS = P (dP - rowsum(P dP)) / sqrt(d) (the gradient at the raw scores q k^T), dQ = dS K, dK = dS^T Q."""
    r = attention_bwd_f16_model(q, k, v, dO, rounding=False)
    return r["dq"], r["dk"], r["dv"], r["p"], r["ds"]


def heads_of(rows, B, T, heads, dm):
    """[B*T, n*heads*dm] (q | k | v | ... side by side) -> n tensors [B, heads, T, dm]."""
    n = rows.shape[1] // (heads * dm)
    x = rows.reshape(B, T, n, heads, dm)
    return tuple(x[:, :, i].permute(0, 2, 1, 3) for i in range(n))


def rows_of(*parts):
    """The inverse of ``heads_of``: n tensors [B, heads, T, dm] -> [B*T, n*heads*dm]."""
    B, heads, T, dm = parts[0].shape
    return torch.cat([t.permute(0, 2, 1, 3).reshape(B * T, heads * dm) for t in parts], 1)
