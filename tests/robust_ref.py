"""CPU restatement of Captum's FGSM and PGD for tests/test_robust_cpu.py and tests/test_gpu_robust.py (captum is absent): the
expressions of Captum 0.7's ``robust/_core/fgsm.py`` (``_perturb``, ``bound``) and ``pgd.py`` (``_clip``, ``_random_point``, the
loop of ``perturb``).

``step`` is the numpy model of advh_robust_step, one fp32 rounding per product, sum and difference, in the order of the torch
expressions (``torch_step`` below, which test_robust_cpu.py holds it to bit for bit); its L2 row norm is taken in float64, so an
L2 result is a bound's centre, not a bit pattern.  ``random_start`` is the model of advh_robust_random_start on the Philox words
of ``attribution_baselines_ref`` and the uniforms of ``metrics_ref``.  ``fgsm`` / ``pgd`` are Captum's loops in torch over the
oracle (``oracle.attribution_ref.input_gradient`` / ``model_logit``); the loss is binary cross-entropy with logits, whose
derivative ``sigmoid(logit) - target`` multiplies the logit's input gradient, as on the device.  Both take ``grad_fn(k, x) ->
dL/dx`` in place of the oracle's gradient, so that a device trace can be replayed or an error model injected."""
import numpy as np
import torch

import attribution_baselines_ref as R
import metrics_ref as MR
from oracle import attribution_ref as A

F = np.float32
ZERO_THRESH = 10 ** -6                                     # FGSM.zero_thresh


def renorm(d, radius):
    """``torch.renorm(d, 2, 0, radius)`` with the row norm in float64: rows longer than ``radius`` are scaled by
    ``radius / (norm + 1e-7)``, the factor rounded to float32 before the float32 product."""
    s = np.sqrt((d.astype(np.float64) ** 2).sum(1))
    fac = np.where(s > F(radius), np.float64(F(radius)) / (s + 1e-7), 1.0).astype(F)
    return d * fac[:, None]


def step(x0, x, g, seed, mask, eps, mult, radius, norm, lo, hi):
    """advh_robust_step on expanded rows: ``x``, ``g`` ``[R, n]``, ``x0 [R, n]`` (unused when ``norm == 0``), ``seed [R]`` or None,
    ``mask`` broadcastable to ``[R, n]`` or None, ``eps`` a number or ``[R]`` numbers, ``mult`` +1 / -1, ``norm`` 0 (none), 1
    (Linf), 2 (L2).  Returns ``[R, n]`` float32."""
    x, g = np.asarray(x, F), np.asarray(g, F)
    gl = g if seed is None else np.asarray(seed, F).reshape(-1, 1) * g
    e = (mult * np.asarray(eps, np.float64)).astype(F).reshape(-1, 1)      # the product in double (a Python float), then fp32
    t = e * np.sign(gl)
    if mask is not None:
        t = t * np.asarray(mask, F)
    v = np.where(np.abs(gl) > F(ZERO_THRESH), x + t, x)
    if norm == 1:
        x0 = np.asarray(x0, F)
        v = x0 + np.minimum(np.maximum(v - x0, F(-radius)), F(radius))
    elif norm == 2:
        x0 = np.asarray(x0, F)
        v = x0 + renorm(v - x0, radius)
    elif norm != 0:
        raise AssertionError(norm)
    return np.minimum(np.maximum(v, F(lo)), F(hi))


def torch_step(x0, x, g, eps, mult, radius, norm, lo, hi, mask=None):
    """Captum's own expressions on torch CPU tensors: ``FGSM._perturb`` (``g`` the loss gradient), ``PGD._clip`` (``norm`` None,
    "Linf" or "L2") and ``bound``."""
    m = 1 if mask is None else mask
    v = torch.where(torch.abs(g) > ZERO_THRESH, x + mult * eps * torch.sign(g) * m, x)
    if norm is not None:
        diff = v - x0
        if norm == "Linf":
            v = x0 + torch.clamp(diff, -radius, radius)
        elif norm == "L2":
            v = x0 + torch.renorm(diff, 2, 0, radius)
        else:
            raise AssertionError("Norm constraint must be L2 or Linf.")
    return torch.clamp(v, min=lo, max=hi)


def first_uniform(seed, row0, rows):
    """u of the first Philox word of rows ``[row0, row0 + rows)``, float32 (exact)."""
    w = R.philox_words(seed, row0, rows, 4).reshape(rows, -1)[:, 0]
    return ((w >> np.uint32(9)).astype(F) * F(2) + F(1)) * F(2.0 ** -24)


def random_start(x0, seed, norm, radius, lo, hi):
    """advh_robust_random_start.  Linf (``norm == 1``): float32 rows, the device's bits.  L2 (``norm == 2``): ``(rows, r)`` in
    float64, ``r[b] = radius * u_b ** (1 / n)`` the row's distance from ``x0`` before the bounds."""
    x0 = np.asarray(x0, F)
    B, n = x0.shape
    if norm == 1:
        v = x0 + F(radius) * MR.uniform(seed, 0, B, n)
        return np.minimum(np.maximum(v, F(lo)), F(hi))
    z = np.asarray(R.philox_normal(seed, 0, B, n), np.float64)
    r = np.float64(F(radius)) * first_uniform(seed, B, B).astype(np.float64) ** (1.0 / n)
    v = x0.astype(np.float64) + (r / np.sqrt((z * z).sum(1)))[:, None] * z
    return np.minimum(np.maximum(v, lo), hi), r


def loss_seed(x, target, model):
    """``sigmoid(logit) - target`` per clip, ``[B]`` float32: d BCE-with-logits / d logit."""
    t = target.reshape(-1).float() if torch.is_tensor(target) else float(target)
    with torch.no_grad():
        return torch.sigmoid(A.model_logit(x, *model).reshape(-1)) - t


def loss_gradient(x, target, model):
    """dL/dx of the summed BCE-with-logits: the per-clip seed times the logit's input gradient."""
    return loss_seed(x, target, model)[:, None] * A.input_gradient(x, *model)


def bce(x, target, model):
    """Per-clip binary cross-entropy with logits of the oracle at ``x``, ``[B]`` float64."""
    t = (target.reshape(-1) if torch.is_tensor(target) else torch.full((x.shape[0],), float(target))).double()
    with torch.no_grad():
        z = A.model_logit(x, *model).reshape(-1).double()
    return torch.nn.functional.binary_cross_entropy_with_logits(z, t, reduction="none")


def fgsm(x, epsilon, target, model, targeted=False, mask=None, lo=-np.inf, hi=np.inf, grad_fn=None):
    """Captum's ``FGSM.perturb``."""
    g = loss_gradient(x, target, model) if grad_fn is None else grad_fn(0, x)
    return torch_step(None, x, g, epsilon, -1 if targeted else 1, None, None, lo, hi, mask)


def pgd(x, radius, step_size, step_num, target, model, targeted=False, start=None, norm="Linf", mask=None, lo=-np.inf, hi=np.inf,
        grad_fn=None):
    """Captum's ``PGD.perturb``; ``start`` is the (already bounded) random start, or None."""
    cur = x if start is None else start
    for k in range(step_num):
        g = loss_gradient(cur, target, model) if grad_fn is None else grad_fn(k, cur)
        cur = torch_step(x, cur, g, step_size, -1 if targeted else 1, radius, norm, lo, hi, mask)
    return cur
