"""CPU restatement of Captum's ShapleyValueSampling, ShapleyValues and KernelShap for tests/test_shapley_cpu.py and
tests/test_gpu_shapley.py, written the way Captum computes them (captum is absent; restated from
``captum.attr._core.shapley_value`` and ``lime`` / ``kernel_shap``).

Shapley: for each permutation, ``prev = F(baseline)``; step j ORs the 0/1 mask of feature ``perm[j]`` into the current mask,
evaluates ``baseline * (1 - m) + x * m``, and adds ``(F(current) - prev) * mask_j`` to ``total``; at the end ``total / P``.
KernelShap: per clip, the interpretable inputs ``z`` (given), inputs ``baseline * (1 - m) + x * m`` with ``m = z[feature]``,
and sklearn's ``LinearRegression().fit(z, y, sample_weight=w)`` (centre by the weighted means, scale the rows by sqrt(w),
``lstsq``, intercept = y_offset - x_offset . coef) with Captum's similarity weights (1e6 for the empty and the full coalition).

Features are given as an index map ``[1 | B, L]`` in ``[0, K)`` (the engine's ranks of the ids present); permutations as
``perm [P, K]`` (``perm[p][j]`` the feature switched at step j).  The forward is pluggable as in ``ablation_ref``: a callable
``[rows, L] -> [rows]`` logits, or given logits ``fbase [B]`` and ``fk`` (row ``(p * K + j) * B + b``; KernelShap:
``y [S, B]``)."""
import itertools

import numpy as np
import torch

from ablation_ref import model_forward  # noqa: F401  (re-exported: the oracle's CPU forward)


def _baseline(base, L):
    return torch.full((1, L), float(base)) if isinstance(base, (int, float)) else base.to(torch.float32)


def feature_mask_of(index, k, B, L):
    """Captum's per-feature 0/1 mask ``[B, L]`` of feature k."""
    return (index == k).to(torch.float32).expand(B, L)


def coalition_row(x, base, m):
    """``baseline * (1 - m) + x * m`` for a 0/1 mask ``m [B, L]``."""
    return base.expand_as(x) * (1 - m) + x * m


def permutation_rows(x, base, index, perm):
    """``[P * K * B, L]`` rows, row ``(p * K + j) * B + b``: the features ``perm[p][:j + 1]`` from x, the rest baseline."""
    B, L = x.shape
    base = _baseline(base, L)
    out = []
    for p in perm:
        m = torch.zeros(B, L)
        for k in p:
            m = torch.maximum(m, feature_mask_of(index, int(k), B, L))
            out.append(coalition_row(x, base, m))
    return torch.cat(out)


def shapley(x, base, index, perm, forward=None, fbase=None, fk=None):
    """Captum's ShapleyValueSampling / ShapleyValues loop over the permutations ``perm [P, K]``: ``attr [B, L]`` fp32."""
    B, L = x.shape
    base = _baseline(base, L)
    P, K = len(perm), len(perm[0])
    if forward is not None:
        fbase = forward(base.expand(B, L).contiguous()).view(-1)
        fk = forward(permutation_rows(x, base, index, perm)).view(-1)
    fk = fk.view(P, K, B)
    total = torch.zeros(B, L)
    for p in range(P):
        prev = fbase
        for j in range(K):
            cur = fk[p, j]
            total += (cur - prev)[:, None] * feature_mask_of(index, int(perm[p][j]), B, L)
            prev = cur
    return total / P


def all_permutations(K):
    """ShapleyValues' permutations, ``itertools.permutations`` order, ``[K!, K]``."""
    return np.array(list(itertools.permutations(range(K))), dtype=np.int64)


def kernel_weights(z):
    n = z.sum(1)
    return np.where((n == 0) | (n == z.shape[1]), 1e6, 1.0)


def linear_regression(z, y, w):
    """sklearn ``LinearRegression(fit_intercept=True).fit(z, y, sample_weight=w)`` in float64: ``(coef, intercept)``."""
    X = np.asarray(z, np.float64)
    y = np.asarray(y, np.float64)
    x_offset = np.average(X, axis=0, weights=w)
    y_offset = np.average(y, weights=w)
    sw = np.sqrt(w)
    Xs = (X - x_offset) * sw[:, None]
    ys = (y - y_offset) * sw
    coef = np.linalg.lstsq(Xs, ys, rcond=None)[0]
    return coef, y_offset - x_offset @ coef


def kernel_shap_rows(x, base, index_b, z_b, b):
    """Clip b's ``[S, L]`` rows: ``m = z_b[s][index_b]``."""
    L = x.shape[1]
    base = _baseline(base, L)
    bb = base[0 if base.shape[0] == 1 else b]
    m = torch.from_numpy(z_b.astype(np.float32))[:, index_b.long()]
    return bb[None] * (1 - m) + x[b][None] * m


def kernel_shap(x, base, index, z, forward=None, y=None):
    """Captum's KernelShap of ``x [B, L]`` (each clip fitted on its own): ``index [1 | B, L]`` per-clip feature ranks, ``z``
    per clip ``[S, K_b]``.  Returns ``(attr [B, L] fp32, coefs, intercepts)``."""
    B, L = x.shape
    attr = torch.zeros(B, L)
    coefs, icpts = [], []
    for b in range(B):
        ib = index[0 if index.shape[0] == 1 else b]
        yb = forward(kernel_shap_rows(x, base, ib, z[b], b)).view(-1).double().numpy() if forward is not None else y[:, b]
        coef, icpt = linear_regression(z[b], yb, kernel_weights(z[b]))
        for k in range(coef.shape[0]):                      # Captum's _convert_output_shape: += coef.item() * (mask == k)
            attr[b] += float(coef[k]) * (ib == k).to(torch.float32)
        coefs.append(coef)
        icpts.append(icpt)
    return attr, coefs, np.array(icpts)
