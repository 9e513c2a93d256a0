"""CPU restatement of Captum's Lime and FeaturePermutation for tests/test_lime_cpu.py and tests/test_gpu_lime.py, written the
way Captum computes them (captum is absent; restated from ``captum.attr._core.lime`` / ``feature_permutation`` and
``captum._utils.models.linear_model``).

FeaturePermutation: for feature k, ``x[perm] * m + x * (1 - m)`` with ``m`` the feature's 0/1 mask (Captum's
``_permute_feature``), rows perturbation-major ``k * B + b``; ``attr = F(x)[b] - F(row k(t), b)``.
Lime: the perturbed row of an interpretable sample ``z`` is ``baseline * (1 - m) + x * m`` with ``m = z[feature]`` (KernelShap's
rows, ``shapley_ref.kernel_shap_rows``), its weight ``exp(-d^2 / (2 w^2))`` with Captum's distances in float64, and the fit
is sklearn's weighted Lasso; the checks below state its optimality (KKT) and its local linear map on the active set."""
import numpy as np
import torch

from ablation_ref import model_forward  # noqa: F401  (re-exported: the oracle's CPU forward)
from shapley_ref import kernel_shap_rows  # noqa: F401  (Lime's rows are KernelShap's presence rows)


def permuted_rows(x: np.ndarray, index: np.ndarray, perm: np.ndarray) -> np.ndarray:
    """``[K * B, L]`` float32: row ``k * B + b`` is ``x[b]`` with the samples of feature k (``index == k``) from ``x[perm[k][b]]``."""
    K, B = perm.shape
    out = np.empty((K * B, x.shape[1]), np.float32)
    for k in range(K):
        m = (index.reshape(-1) == k)[None]
        out[k * B:(k + 1) * B] = np.where(m, x[perm[k]], x)
    return out


def feature_permutation(x, index, perm, forward=None, f0=None, fk=None):
    """Captum's FeaturePermutation of ``x [B, L]`` given ``perm [K, B]``: ``attr [B, L]`` fp32 (``f0 - fk`` in fp32)."""
    B, L = x.shape
    K = perm.shape[0]
    if forward is not None:
        f0 = forward(x).view(-1)
        fk = forward(torch.from_numpy(permuted_rows(x.numpy(), index.numpy(), perm))).view(-1)
    fk = fk.view(K, B)
    attr = torch.zeros(B, L)
    idx = index.reshape(-1).long()
    for k in range(K):
        attr += (f0 - fk[k])[:, None] * (idx == k).to(torch.float32)[None]
    return attr


def similarity(x, v, mode: str, width: float) -> float:
    """Captum's ``get_exp_kernel_similarity_function(mode, width)`` in float64: cosine as ``torch.nn.CosineSimilarity(dim=0)``
    (each norm clamped at 1e-8, so a zero row has cos = 0), euclidean ``torch.norm(x - v)``."""
    a = torch.as_tensor(x, dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    if mode == "cosine":
        na = torch.clamp(torch.linalg.vector_norm(a), min=1e-8)
        nb = torch.clamp(torch.linalg.vector_norm(b), min=1e-8)
        d = 1.0 - float(((a / na) * (b / nb)).sum())
    else:
        d = float(torch.linalg.vector_norm(a - b))
    return float(np.exp(-d * d / (2.0 * width * width)))


def centred(z, y, w):
    z = np.asarray(z, np.float64)
    y = np.asarray(y, np.float64)
    w = np.asarray(w, np.float64)
    zm = np.average(z, axis=0, weights=w)
    ym = np.average(y, weights=w)
    return z - zm, y - ym, w / w.sum()


def lasso_gradient(z, y, w, coef, intercept):
    """``g_k = -(1 / sum w) sum_s w_s z_sk (y_s - b - z_s . c)`` of the smooth part of sklearn's weighted Lasso objective, and the
    intercept's own optimality residual ``sum_s w_s r_s / sum w``."""
    z = np.asarray(z, np.float64)
    y = np.asarray(y, np.float64)
    wn = np.asarray(w, np.float64) / np.sum(w)
    r = y - intercept - z @ coef
    return -(wn * r) @ z, float(wn @ r)


def kkt_violation(z, y, w, alpha, coef, intercept):
    """The largest violation of the Lasso's optimality conditions, relative to alpha: ``|g_k + alpha sign c_k|`` for ``c_k != 0``,
    ``max(0, |g_k| - alpha)`` for ``c_k == 0``, and the intercept's residual."""
    g, r0 = lasso_gradient(z, y, w, coef, intercept)
    on = coef != 0
    v_on = np.abs(g[on] + alpha * np.sign(coef[on])).max(initial=0.0)
    v_off = np.maximum(np.abs(g[~on]) - alpha, 0).max(initial=0.0)
    return max(v_on, v_off, abs(r0)) / alpha


def active_set_map(z, w, coef) -> np.ndarray:
    """The Lasso's coefficients on the active set A as a function of y, for fixed signs: ``c_A = M y - const`` with ``M =
    (Z_A^T W Z_A)^-1 Z_A^T W C`` (Z centred by the weighted means, W = diag(w / sum w), C the centring map of y).  Returns M
    ``[|A|, S]``; ``||M||_inf`` bounds how far logit errors move the fit."""
    zc, _, wn = centred(z, np.zeros(len(w)), w)
    A = np.flatnonzero(coef)
    S = zc.shape[0]
    if A.size == 0:
        return np.zeros((0, S))
    ZA = zc[:, A]
    C = np.eye(S) - np.outer(np.ones(S), wn)
    return np.linalg.solve(ZA.T @ (wn[:, None] * ZA), ZA.T @ (wn[:, None] * C))
