"""CPU restatement of the influence methods (Captum 0.7's ``captum.influence``: SimilarityInfluence, TracInCPFast; influence
functions, Koh & Liang 2017) for tests/test_influence_cpu.py and tests/test_gpu_influence.py, in float64 numpy and driven by the
oracle: hidden states from ``layer_attr_ref.hidden``, pooled features as their time mean at the last layer.  Parity with Captum
is unpinned (captum is absent): the formulas are restated from its source and the two papers.

The classifier's trainable part is the logistic regression ``z = coef . phi + intercept`` on pooled features; ``Xa = [phi, 1]``
is the augmented feature matrix and ``v = [coef, intercept]``."""
import numpy as np
import torch

import concept_ref as CR
import layer_attr_ref as LR
from addvisor_hip import synthetic as syn


def sigmoid(z):
    return np.exp(-np.logaddexp(0.0, -np.asarray(z, np.float64)))


def augment(phi):
    phi = np.asarray(phi, np.float64)
    return np.concatenate([phi, np.ones((len(phi), 1))], 1)


def losses(Xa, y, v):
    """BCE-with-logits per sample."""
    z = Xa @ v
    return np.logaddexp(0.0, z) - y * z


def reg_vector(F1, l2):
    r = np.full(F1, float(l2))
    r[-1] = 0.0                                                              # the intercept is not penalised
    return r


def hessian(Xa, v, l2, damping=0.0, weights=None):
    """``(1/N) sum_i w_i p_i (1 - p_i) x_i x_i^T + l2 diag(1, ..., 1, 0) + damping I`` (N = the number of rows)."""
    p = sigmoid(Xa @ v)
    w = p * (1.0 - p) * (1.0 if weights is None else weights)
    return (Xa * w[:, None]).T @ Xa / len(Xa) + np.diag(reg_vector(Xa.shape[1], l2) + damping)


def newton_fit(Xa, y, l2, weights=None, tol=1e-13, max_iter=100, return_iterations=False):
    """The minimiser of ``(1/N) sum_i w_i BCE_i(v) + (l2 / 2) |coef|^2`` by damped Newton from 0, float64."""
    N, F1 = Xa.shape
    w = np.ones(N) if weights is None else np.asarray(weights, np.float64)
    reg = reg_vector(F1, l2)
    obj = lambda u: float(w @ losses(Xa, y, u) / N + 0.5 * reg @ (u * u))
    v = np.zeros(F1)
    J = obj(v)
    for it in range(1, max_iter + 1):
        grad = (w * (sigmoid(Xa @ v) - y)) @ Xa / N + reg * v
        step = -np.linalg.solve(hessian(Xa, v, l2, weights=w), grad)
        t = 1.0
        while obj(v + t * step) > J + 1e-13 * abs(J) and t > 1e-6:
            t *= 0.5
        v = v + t * step
        J = obj(v)
        if t == 1.0 and np.abs(step).max() <= tol:
            break
    return (v, it) if return_iterations else v


def influence_functions(Xn, yn, Xt, yt, v, l2, damping=0.0, hess=None):
    """``S[t, n] = +grad l(test_t)^T H^-1 grad l(train_n)`` (Captum's sign; ``-1 x`` Koh & Liang's ``I_up,loss``), ``[B, N]``.
    ``hess``: another Hessian in place of ``hessian(Xn, v, l2, damping)``."""
    Hm = hessian(Xn, v, l2, damping) if hess is None else hess
    gn = (sigmoid(Xn @ v) - yn)[:, None] * Xn
    gt = (sigmoid(Xt @ v) - yt)[:, None] * Xt
    return gt @ np.linalg.solve(Hm, gn.T)


def gd_checkpoints(Xa, y, l2, lrs):
    """Gradient-descent iterates from 0 on the objective: ``[(v_k, lr_k)]``, ``v_k`` the iterate after the step taken with
    ``lr_k`` (the start, 0, is no checkpoint: it gives p = 1/2 everywhere)."""
    reg = reg_vector(Xa.shape[1], l2)
    v = np.zeros(Xa.shape[1])
    out = []
    for lr in lrs:
        v = v - lr * ((sigmoid(Xa @ v) - y) @ Xa / len(y) + reg * v)
        out.append((v.copy(), float(lr)))
    return out


def tracin(Xn, yn, Xt, yt, checkpoints):
    """``S[t, n] = sum_c lr_c grad l_c(test_t) . grad l_c(train_n)`` over the final linear layer (weights and bias), ``[B, N]``."""
    S = np.zeros((len(Xt), len(Xn)))
    for v, lr in checkpoints:
        gn = (sigmoid(Xn @ v) - yn)[:, None] * Xn
        gt = (sigmoid(Xt @ v) - yt)[:, None] * Xt
        S += lr * (gt @ gn.T)
    return S


def tracin_self(Xn, yn, checkpoints):
    return sum(lr * ((sigmoid(Xn @ v) - yn) ** 2) * (Xn * Xn).sum(1) for v, lr in checkpoints)


def cosine_similarity(X, Y):
    """Captum's ``cosine_similarity`` with ``replace_nan = 0``: a zero row gives 0."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    nx, ny = np.sqrt((X * X).sum(1)), np.sqrt((Y * Y).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        S = (X @ Y.T) / (nx[:, None] * ny[None])
    S[(nx == 0)[:, None] | (ny == 0)[None]] = 0.0
    return S


def euclidean_distance(X, Y):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    return np.sqrt(np.stack([((x[None] - Y) ** 2).sum(1) for x in X]))


def topk(S, k, largest=True):
    """``(indices [M, k], values [M, k])``: ``np.argsort(-+S[m], kind="stable")[:k]``."""
    S = np.asarray(S)
    idx = np.stack([np.argsort(-row if largest else row, kind="stable")[:k] for row in S])
    return idx, np.take_along_axis(S, idx, 1)


def layer_features(h, pool):
    h = h.double().numpy()
    return h.mean(1) if pool == "mean" else h.reshape(len(h), -1)


# ---- the shared case -------------------------------------------------------------------------------------------------------------
L, N_TRAIN, N_TEST = 16000, 40, 6
LAYERS = (0, 4)
L2S = (1.0, 0.1)
LRS = (0.5, 0.25, 0.125)                                                         # the three TracIn checkpoints' learning rates
case_model = CR.case_model


def train_clips():
    return syn.make_clips(N_TRAIN, L, seed=101)


def test_clips():
    return syn.make_clips(N_TEST, L, seed=12)


def train_labels():
    return (np.arange(N_TRAIN) % 2).astype(np.float64)


def test_labels():
    return (np.arange(N_TEST) % 2).astype(np.float64)


_CASE = {}


def case(stable):
    """The oracle's view of the case, computed once per flavour and shared; callers must not modify it: hidden states of the
    requested layers, augmented pooled features ``Xn [40, H + 1]`` / ``Xt [6, H + 1]``, labels, ``theta[l2]`` (the float64 Newton
    minimiser) and the three TracIn ``checkpoints`` (gradient descent at ``l2 = 0.1``)."""
    if stable not in _CASE:
        model = case_model(stable)
        nl = LR.num_layers(model[1])
        hn, ht = LR.hidden(train_clips(), model), LR.hidden(test_clips(), model)
        c = dict(hn={l: hn[l] for l in LAYERS}, ht={l: ht[l] for l in LAYERS}, yn=train_labels(), yt=test_labels(),
                 Xn=augment(hn[nl].double().numpy().mean(1)), Xt=augment(ht[nl].double().numpy().mean(1)))
        c["theta"] = {l2: newton_fit(c["Xn"], c["yn"], l2) for l2 in L2S}
        c["checkpoints"] = gd_checkpoints(c["Xn"], c["yn"], 0.1, LRS)
        _CASE[stable] = c
    return _CASE[stable]
