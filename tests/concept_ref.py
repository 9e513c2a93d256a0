"""CPU restatement of TCAV (Kim et al. 2018; Captum 0.7's ``captum.concept.TCAV``) for tests/test_concept_cpu.py and
tests/test_gpu_concept.py, in float64 and driven by the oracle: activations from ``layer_attr_ref.hidden``, gradients from
``layer_attr_ref.layer_gradient`` (fp32 autograd on the oracle's encoder), and the logistic CAV solved in the PRIMAL by Newton
on ``(w, b)`` -- a different route from the engine's dual solve on the Gram matrix.  Parity with Captum is unpinned (captum is
absent): the formulas are restated.

``model`` is ``(sd, cfg, coef, intercept)`` as in tests/layer_attr_ref.py."""
import math

import numpy as np
import torch

import layer_attr_ref as LR
from addvisor_hip import synthetic as syn


def sig_neg(z):
    return np.exp(-np.logaddexp(0.0, z))


def logistic_primal(X, y, alpha, tol=1e-13, max_iter=100):
    """The minimiser ``(w [F], b)`` of ``(1/n) sum log(1 + exp(-y_i (w . x_i + b))) + (alpha / 2) ||w||^2``: damped Newton on
    the ``F + 1`` primal unknowns, float64."""
    X, y = np.asarray(X, np.float64), np.asarray(y, np.float64)
    n, F = X.shape
    if F > n:
        # w lies in the span of the rows: with X^T = Q R (Q [F, n] orthonormal) and w = Q z, ||w|| = ||z|| and X w = R^T z -- the
        # same primal problem in n unknowns (an exact change of variables; it never forms X X^T)
        Q, R = np.linalg.qr(X.T)
        z, b = logistic_primal(R.T, y, alpha, tol, max_iter)
        return Q @ z, b
    Xe = np.concatenate([X, np.ones((n, 1))], 1)
    reg = np.concatenate([np.full(F, alpha), [0.0]])
    v = np.zeros(F + 1)

    def obj(v):
        return np.logaddexp(0.0, -y * (Xe @ v)).mean() + 0.5 * float(reg @ (v * v))

    J = obj(v)
    for _ in range(max_iter):
        s = sig_neg(y * (Xe @ v))
        grad = reg * v - (y * s) @ Xe / n
        Hm = (Xe * (s * (1 - s))[:, None]).T @ Xe / n + np.diag(reg)
        try:
            step = -np.linalg.solve(Hm, grad)
        except np.linalg.LinAlgError:
            step = -np.linalg.lstsq(Hm, grad, rcond=None)[0]
        t = 1.0
        while obj(v + t * step) > J + 1e-13 * abs(J) and t > 1e-6:
            t *= 0.5
        v = v + t * step
        J = obj(v)
        if t == 1.0 and np.abs(step).max() <= tol:
            break
    return v[:F], float(v[F])


def primal_gradient(X, y, w, b, alpha):
    """``(max |alpha w - (1/n) sum y_i s_i x_i|, |sum y_i s_i|)``, ``s_i = sigma(-y_i (w . x_i + b))``."""
    s = sig_neg(y * (X @ w + b))
    return np.abs(alpha * w - (y * s) @ X / len(y)).max(), abs(float((y * s).sum()))


def split_rows(n, ratio, seed):
    perm = np.random.default_rng(seed).permutation(n)
    k = int(ratio * n)
    return perm[k:], perm[:k]


def fit_cav(feats, alpha=0.01, ratio=0.33, seed=0, classifier="logistic"):
    """``feats``: one ``[n_c, F]`` float64 matrix per concept.  Returns ``(weights [C, F], intercepts [C], acc)`` with Captum's
    two-concept rows ``[-w, w]`` and one-vs-rest beyond."""
    X = np.concatenate(feats)
    labels = np.concatenate([np.full(len(f), i) for i, f in enumerate(feats)])
    train, test = split_rows(len(X), ratio, seed)
    C = len(feats)

    def one(c):
        y = np.where(labels[train] == c, 1.0, -1.0)
        if classifier == "logistic":
            return logistic_primal(X[train], y, alpha)
        mp, mn = X[train][y > 0].mean(0), X[train][y < 0].mean(0)
        return mp - mn, float(-0.5 * (mp - mn) @ (mp + mn))

    if C == 2:
        w, b = one(1)
        W, bs = np.stack([-w, w]), np.array([-b, b])
    else:
        fits = [one(c) for c in range(C)]
        W, bs = np.stack([f[0] for f in fits]), np.array([f[1] for f in fits])
    ev = test if len(test) else train
    m = X[ev] @ W.T + bs
    pred = (m[:, 1] > 0).astype(int) if C == 2 else m.argmax(1)
    return W, bs, float((pred == labels[ev]).mean())


def scores_of(s, magnitude="mean"):
    s = np.asarray(s, np.float64)
    sign = (s > 0).mean(0)
    return sign, (s.mean(0) if magnitude == "mean" else np.abs(s * (s > 0)).sum(0) / np.abs(s).sum(0))


def features(h, pool):
    h = h.double().numpy()
    return h.mean(1) if pool == "mean" else h.reshape(len(h), -1)


def tcav(model, concepts, sets, inputs, layers, pool="none", alpha=0.01, ratio=0.33, seed=0, cache=None):
    """``concepts``: ``{id: waves [n, L]}``; ``sets``: lists of ids.  Returns ``{"0-1": {layer: dict(weights, intercepts, accs,
    scores [B, C], sign_count, magnitude, grad)}}``, everything float64 numpy.  ``cache``: a dict that keeps the oracle's hidden
    states and gradients between calls that differ in ``pool`` alone."""
    cache = {} if cache is None else cache
    if "hidden" not in cache:
        cache["hidden"] = {cid: LR.hidden(w, model) for cid, w in concepts.items()}
        hx = LR.hidden(inputs, model)
        cache["grad"] = {l: LR.layer_gradient(hx[l], l, model).double().numpy() for l in layers}      # [B, T, H]
    out = {}
    for l in layers:
        feats = {cid: features(hs[l], pool) for cid, hs in cache["hidden"].items()}
        g = cache["grad"][l]
        gx = g.sum(1) if pool == "mean" else g.reshape(len(g), -1)
        for s in sets:
            W, b, acc = fit_cav([feats[c] for c in s], alpha, ratio, seed)
            sc = gx @ W.T
            sign, mag = scores_of(sc)
            out.setdefault("-".join(str(c) for c in s), {})[l] = dict(weights=W, intercepts=b, accs=acc, scores=sc, sign_count=sign,
                                                                      magnitude=mag, grad=g)
    return out


# ---- the shared case of the engine parity tests -------------------------------------------------------------------------------
L, N_CLIPS, N_INPUTS = 16000, 12, 8
LAYERS = (0, 4)
SETS = ([0, 1], [2, 1])                                                          # A / R1 and R2 / R1


def case_concepts():
    """Concept 0 = clips plus a 3 kHz tone of amplitude 0.2; concepts 1 and 2 = random clip sets."""
    t = torch.arange(L, dtype=torch.float64) / 16000.0
    tone = (0.2 * torch.sin(2 * math.pi * 3000.0 * t)).float()
    return {0: syn.make_clips(N_CLIPS, L, seed=101) + tone, 1: syn.make_clips(N_CLIPS, L, seed=202), 2: syn.make_clips(N_CLIPS, L, seed=303)}


def case_inputs():
    return syn.make_clips(N_INPUTS, L, seed=12)


def case_model(stable):
    cfg = syn.tiny_config(stable)
    coef, icpt = syn.logreg_weights(cfg.hidden_size)
    return syn.embedder_weights(cfg), cfg, coef, icpt


_CASE, _ORACLE = {}, {}


def case_reference(stable, pool):
    """Computed once per (flavour, pool) and shared; callers must not modify it."""
    key = (stable, pool)
    if key not in _CASE:
        _CASE[key] = tcav(case_model(stable), case_concepts(), SETS, case_inputs(), LAYERS, pool, cache=_ORACLE.setdefault(stable, {}))
    return _CASE[key]


# ---- the real-valued Gram inputs ------------------------------------------------------------------------------------------------
GRAM_REAL_SHAPES = ((70, 70, 3136), (33, 33, 4099))


def gram_real_inputs(M, F, seed=5):
    """``3 randn + 2`` in fp32 with the first and last columns set to 4.0 (a reference that drops a column must miss the bound)."""
    x = (3.0 * torch.randn(M, F, generator=torch.Generator().manual_seed(seed)) + 2.0).float()
    x[:, 0] = 4.0
    x[:, -1] = 4.0
    return x.numpy()


def gram_error(G, X64, Y64):
    """The largest error of ``G`` per entry relative to ``sum_f |x y|``, against float64."""
    ref = X64 @ Y64.T
    scale = np.abs(X64) @ np.abs(Y64).T
    return float((np.abs(np.asarray(G, np.float64) - ref) / scale).max())


def gram_bound(X32):
    """8 x the error of numpy's own fp32 ``X32 @ X32.T`` against float64 at the same shape (the factor is for the different
    summation order, not for a worse accuracy)."""
    X64 = X32.astype(np.float64)
    return 8.0 * gram_error(X32 @ X32.T, X64, X64)
